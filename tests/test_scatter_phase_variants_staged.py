"""CPU-only: the staged route of JacobianGPU groups states that differ in an aerosol's phase function into ONE batched scattering
call when the engine advertises `scatter_phase_variants`, and keeps today's grouping -- one call per distinct PHASE -- for every
other engine and when the engine refuses the variants."""
import numpy as np
import pytest

from archnemesis_dist_amd.continuum_rows import expand_rows
from test_scatter_rows import _fm, _staged_records


def _spectrum(lt, am, taudust, phasarr, radg):
    """a spectrum that depends on the state's own arrays and on the phase function it was run with -> (W, 1)"""
    return (radg[:, :1] + taudust.sum(axis=1)[:, None] * lt.sum() + am.sum() + phasarr[0, :, 0, :1] * 7.0 + phasarr[1, :, 0, 1:2])


class _Recorder:
    """`cirsrad_ck_scatter_batch_rows` and the dense entry of an engine without per-model phase functions"""

    def __init__(self):
        self.calls = []

    def _run(self, entry, lt, am, taudust, phasarr, radg, kw):
        n = lt.shape[0]
        self.calls.append(dict(entry=entry, n=n, phasarr=np.array(phasarr), kw=dict(kw), lt=np.array(lt)))
        phase_of = kw.get("phase_of")
        variants = [np.asarray(phasarr)] + ([] if phase_of is None else list(kw["phasarr_variants"]))
        of = np.zeros(n, dtype=int) if phase_of is None else np.asarray(phase_of)
        return np.stack([_spectrum(lt[m], am[m], taudust[m], variants[of[m]], radg[m]) for m in range(n)])

    def cirsrad_ck_scatter_batch_rows(self, ISPACE, lp, lt, am, cont_row, cia, dust, ray, sca, phasarr, lfrac_rows, radg, *rest, **kw):
        assert len(rest) == 12
        return self._run("rows", lt, am, expand_rows(cont_row, dust)[0], phasarr, radg, kw)

    def cirsrad_ck_scatter_batch(self, ISPACE, lp, lt, am, cia, dust, ray, sca, phasarr, lfrac, radg, *rest, **kw):
        assert len(rest) == 12
        return self._run("dense", lt, am, dust, phasarr, radg, kw)


class _WithVariants(_Recorder):
    scatter_phase_variants = True


class _Refuses(_WithVariants):
    """advertises the keywords and refuses them, as the library does for a slice, one g-ordinate or no room"""

    def _run(self, entry, lt, am, taudust, phasarr, radg, kw):
        if kw.get("phase_of") is not None:
            self.calls.append(dict(entry=entry, refused=True))
            raise NotImplementedError("cirsrad_ck_scatter_batch: ANSFM_ERR_UNSUPPORTED")
        return super()._run(entry, lt, am, taudust, phasarr, radg, kw)


def _records():
    """five states of one geometry: PHASE A, B, A, C, B (three different arrays, in that order of first appearance)"""
    recs, W = _staged_records(1)
    A = recs[0]["PHASE"].copy()
    B = A.copy(); B[0, :, 0, 0] = 2.0
    C = A.copy(); C[1, 2:, 0, 1] = 3.0
    for r, ph in zip(recs, (A, B, A, C, B)):
        r["PHASE"] = ph.copy()
    return recs, W, (A, B, C)


def _want(recs):
    return [_spectrum(r["lt"], r["f_gas"], r["TAUDUST"], r["PHASE"], r["RADGROUND"]) for r in recs]


def _run(eng, rows):
    fm = _fm()
    recs, W, phases = _records()
    want = _want(recs)
    if rows:
        packers = {}
        for r in recs:
            fm._ansfm_pack_scatter(r, packers, variants=fm._ansfm_phase_variants(eng))
    got, _, _ = fm._ansfm_run_batches(eng, recs, W)
    assert len(got) == 5
    for k in range(5):
        assert np.array_equal(got[k], want[k]), k
    assert len({g.tobytes() for g in got}) == 5               # no state's spectrum could stand in for another's
    return phases


@pytest.mark.parametrize("rows", [True, False])
def test_engine_with_variants_gets_one_call(rows):
    eng = _WithVariants()
    A, B, C = _run(eng, rows)
    assert len(eng.calls) == 1
    c = eng.calls[0]
    assert c["entry"] == ("rows" if rows else "dense") and c["n"] == 5
    assert np.array_equal(c["phasarr"], A)                                   # the first state's
    assert c["kw"]["phase_of"].tolist() == [0, 1, 0, 2, 1] and c["kw"]["phase_of"].dtype == np.int32
    pv = np.asarray(c["kw"]["phasarr_variants"])
    assert pv.shape == (2,) + A.shape and np.array_equal(pv[0], B) and np.array_equal(pv[1], C)   # in order of first appearance


@pytest.mark.parametrize("rows", [True, False])
def test_engine_without_the_attribute_keeps_todays_three_calls(rows):
    eng = _Recorder()
    A, B, C = _run(eng, rows)
    assert [c["n"] for c in eng.calls] == [2, 2, 1] and all(c["kw"] == {} for c in eng.calls)
    for c, ph in zip(eng.calls, (A, B, C)):
        assert np.array_equal(c["phasarr"], ph)


@pytest.mark.parametrize("rows", [True, False])
def test_refused_variants_fall_back_to_todays_grouping(rows):
    eng = _Refuses()
    A, B, C = _run(eng, rows)
    assert eng.calls[0].get("refused") and len(eng.calls) == 4
    assert [c["n"] for c in eng.calls[1:]] == [2, 2, 1] and all(c["kw"] == {} for c in eng.calls[1:])
    for c, ph in zip(eng.calls[1:], (A, B, C)):
        assert np.array_equal(c["phasarr"], ph)
    recs, _, _ = _records()
    assert np.array_equal(eng.calls[1]["lt"], np.stack([recs[0]["lt"], recs[2]["lt"]]))      # states 0 and 2 run together


def test_states_with_one_phase_function_make_the_plain_call():
    eng = _WithVariants()
    fm = _fm()
    recs, W = _staged_records(1)
    fm._ansfm_run_batches(eng, recs, W)
    assert len(eng.calls) == 1 and eng.calls[0]["kw"] == {}


def test_key_keeps_shape_and_imie_without_the_bytes():
    fm = _fm()
    recs, _, _ = _records()
    key = fm._ansfm_scatter_key
    assert key(recs[0]) != key(recs[1]) and key(recs[0]) == key(recs[2])
    assert key(recs[0], True) == key(recs[1], True) == key(recs[3], True)
    other_shape = dict(recs[1], PHASE=recs[1]["PHASE"][:, :, :, :4])
    other_imie = dict(recs[1], IMIE=1)
    assert key(recs[0], True) != key(other_shape, True) and key(recs[0], True) != key(other_imie, True)
    import archnemesis_dist_amd.engine as engine
    assert engine.AnsfmEngine.scatter_phase_variants is True
