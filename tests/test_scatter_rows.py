"""The batched multiple-scattering branch with the continuum handed over once per distinct layer:
ansfm_cirsrad_ck_scatter_batch_rows (engine: cirsrad_ck_scatter_batch_rows), the packer continuum_rows.ContinuumRows, the
staged Jacobian route and the sharded Jacobian on the rows form.  Everything is compared with np.array_equal against the dense
entry called with the expanded arrays: the arithmetic per (wavenumber, g, layer) is the same, so the bits are."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_scatter_wavenumber_shard import (_ToyEngine, _batch_args, _ktable_case, _ktable_upload, _models, _toy_inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
DENSE = ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac")
ROWS = ("TAUCIA_rows", "TAUDUST_rows", "TAURAY_rows", "TAUSCAT_rows", "lfrac_rows")


# ---- 1. the packer -----------------------------------------------------------------------------------------------------------
def _five_states(W=9, L=12, C=2, seed=11):
    """five states built like _models: a temperature change and a gas change (the continuum stays), TAUDUST of layers 5 - 6
    scaled, a boundary change (the continuum stays)"""
    rng = np.random.default_rng(seed)
    z = dict(lay_p=np.logspace(5, 2, L), lay_t=np.linspace(160, 110, L), amount=rng.uniform(1, 2, (3, L)),
             TAUCIA=rng.uniform(0, 1, (W, L)), TAUDUST=rng.uniform(0, 1, (W, L)), TAURAY=rng.uniform(0, 1, (W, L)),
             TAUSCAT=rng.uniform(0, 1, (W, L)), lfrac=rng.uniform(0, 1, (W, C, L)), radg=rng.uniform(1, 2, (W, 4)))
    return _models(z)


def test_packer_keeps_the_first_state_and_the_changed_layers():
    from archnemesis_dist_amd.continuum_rows import ContinuumRows
    b = _five_states()
    n, W, L = b["TAUDUST"].shape
    pk = ContinuumRows(L, b["lfrac"].shape[2])
    for m in range(n):
        pk.add_state(*(b[k][m] for k in DENSE))
    assert pk.R == L + 2 and pk.n_states == n
    cr = pk.cont_row
    assert cr.dtype == np.int32 and cr.shape == (n, L) and np.array_equal(cr[0], np.arange(L))
    for m in (1, 2, 4):
        assert np.array_equal(cr[m], cr[0])
    assert np.array_equal(cr[3], np.r_[np.arange(5), L, L + 1, np.arange(7, L)])
    assert pk.TAUCIA_rows.shape == (L + 2, W) and pk.lfrac_rows.shape == (L + 2, 2, W)
    assert pk.TAUDUST_rows.flags.c_contiguous and pk.lfrac_rows.flags.c_contiguous
    assert np.array_equal(pk.TAUDUST_rows[L], b["TAUDUST"][3, :, 5]) and np.array_equal(pk.lfrac_rows[3, 1], b["lfrac"][0, :, 1, 3])
    for name, got in zip(DENSE, pk.expand()):
        assert got.shape == b[name].shape and np.array_equal(got.view(np.uint64), b[name].view(np.uint64)), name


def test_packer_compares_bits_not_values():
    """-0.0 against 0.0 and two NaNs with different payloads are equal or unordered as numbers and different as bits: the
    layer is a new row, and expand() gives the bits back"""
    from archnemesis_dist_amd.continuum_rows import ContinuumRows
    W, L = 4, 3
    base = np.zeros((W, L)); base[1, 2] = np.nan
    frac = np.ones((W, 1, L))
    pk = ContinuumRows(L, 1)
    pk.add_state(base, base, None, base, frac)
    neg = base.copy(); neg[2, 0] = -0.0
    assert np.array_equal(neg[:, 0], base[:, 0])                               # equal as numbers
    assert np.array_equal(pk.add_state(base, neg, None, base, frac), [L, 1, 2])
    nan2 = base.copy()
    nan2.view(np.uint64)[1, 2] ^= 1                                            # another payload, still a NaN
    assert np.isnan(nan2[1, 2])
    assert np.array_equal(pk.add_state(base, base, None, nan2, frac), [0, 1, L + 1])
    f2 = frac.copy(); f2[3, 0, 1] = 0.5
    assert np.array_equal(pk.add_state(base, base, None, base, f2), [0, L + 2, 2])
    assert np.array_equal(pk.add_state(base, base, None, base, frac), [0, 1, 2])
    assert pk.R == L + 3 and pk.TAURAY_rows is None
    cia, dust, ray, sca, lf = pk.expand()
    assert ray is None
    assert np.signbit(dust[1, 2, 0]) and not np.signbit(dust[0, 2, 0])
    assert sca.view(np.uint64)[2, 1, 2] == nan2.view(np.uint64)[1, 2] != sca.view(np.uint64)[0, 1, 2]
    assert lf[3, 3, 0, 1] == 0.5 and lf[4, 3, 0, 1] == 1.0


def test_packer_rejects_another_shape_and_a_changing_none():
    from archnemesis_dist_amd.continuum_rows import ContinuumRows
    W, L = 5, 4
    a = np.ones((W, L)); f = np.ones((W, 2, L))
    pk = ContinuumRows(L, 2)
    pk.add_state(a, a, None, a, f)
    with pytest.raises(ValueError):
        pk.add_state(np.ones((W, L + 1)), a, None, a, f)                       # another L
    with pytest.raises(ValueError):
        pk.add_state(a, np.ones((W + 1, L)), None, a, f)                       # another W
    with pytest.raises(ValueError):
        pk.add_state(a, a, None, a, np.ones((W, 3, L)))                        # another NDUST
    with pytest.raises(ValueError):
        pk.add_state(a, a, a, a, f)                                            # TAURAY was None
    with pytest.raises(ValueError):
        pk.add_state(None, a, None, a, f)
    assert pk.n_states == 1 and pk.R == L
    with pytest.raises(ValueError):
        ContinuumRows(L, 2).rows()                                             # nothing added
    nodust = ContinuumRows(L, 0)                                               # no aerosols: FRAC (W, 0, L) or None, no rows of it
    nodust.add_state(a, None, None, None, np.ones((W, 0, L)))
    nodust.add_state(a * 2, None, None, None, None)
    assert nodust.R == 2 * L and nodust.lfrac_rows is None and nodust.TAUDUST_rows is None


# ---- 2. the staged route of the drop-in Jacobian ----------------------------------------------------------------------------
class _DenseDouble:
    """records what the staged route hands to the batched scattering entry; the spectrum of a state is made from its own
    inputs, so that a state routed to the wrong place shows"""

    def __init__(self):
        self.calls = []

    def cirsrad_ck_scatter_batch(self, ISPACE, lp, lt, am, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac, radg, *rest, **kw):
        self.calls.append(dict(ISPACE=ISPACE, lp=lp, lt=lt, am=am, TAUCIA=TAUCIA, TAUDUST=TAUDUST, TAURAY=TAURAY, TAUSCAT=TAUSCAT,
                               phasarr=phasarr, lfrac=lfrac, radg=radg, rest=rest, kw=kw))
        return (TAUDUST.sum(axis=2) + lfrac.sum(axis=(2, 3)) * lt.sum(axis=1)[:, None] + am.sum(axis=(1, 2))[:, None]
                + radg[:, :, 0])[:, :, None]


class _RowsDouble(_DenseDouble):
    def __init__(self):
        super().__init__()
        self.rows_calls = []

    def cirsrad_ck_scatter_batch_rows(self, ISPACE, lp, lt, am, cont_row, cia, dust, ray, sca, phasarr, lfrac_rows, radg, *rest, **kw):
        from archnemesis_dist_amd.continuum_rows import expand_rows
        self.rows_calls.append(dict(cont_row=cont_row, R=dust.shape[0]))
        return _DenseDouble.cirsrad_ck_scatter_batch(self, ISPACE, lp, lt, am, *expand_rows(cont_row, cia, dust, ray, sca)[:4], phasarr,
                                                     expand_rows(cont_row, lfrac_rows)[0], radg, *rest, **kw)


def _same_call(a, b):
    for k in ("ISPACE", "lp", "lt", "am", "TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "phasarr", "lfrac", "radg"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, k
    assert len(a["rest"]) == len(b["rest"]) and a["kw"] == b["kw"]
    for x, y in zip(a["rest"], b["rest"]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def _staged_records(n_geom_groups=2):
    """staged scattering records of five states, as CIRSradGPU._ansfm_cirsrad_scatter(None, ...) leaves them; states 1 and 3 look
    at another angle than the rest (another group of the batched call), so the packers are per group"""
    b = _five_states()
    n, W, L = b["TAUDUST"].shape
    recs = []
    for m in range(n):
        recs.append(dict(scatter=True, ISPACE=0, lp=b["lay_press_pa"][m], lt=b["lay_temp"][m], f_gas=b["amount"][m], TAUCIA=b["TAUCIA"][m],
                         TAUDUST=b["TAUDUST"][m], TAURAY=b["TAURAY"][m], TAUSCAT=b["TAUSCAT"][m], PHASE=np.ones((2, W, 2, 5)),
                         FRAC=b["lfrac"][m], RADGROUND=b["radg"][m], SOL_ANG=np.array([30.0]),
                         EMISS_ANG=np.array([20.0 if m % 2 == 0 or n_geom_groups == 1 else 40.0]), AZI_ANG=np.array([0.0]),
                         solar=np.ones(W), LOWBC=1, BRDF=np.zeros((W, 4, 4, 2)), MU=np.ones(4), WTMU=np.ones(4), NF=1, NPHI=11,
                         IRAY=1, IMIE=0))
    return recs, W


def _fm():
    from archnemesis_dist_amd.jacobian_dropin import JacobianGPU

    class FM(JacobianGPU):
        def _ansfm_upload_table(self, eng):
            pass
    return FM()


@pytest.mark.parametrize("groups", [1, 2])
def test_staged_records_go_through_the_rows_entry_and_back(groups):
    fm = _fm()
    dense_recs, W = _staged_records(groups)
    dense = _DenseDouble()
    want, _, _ = fm._ansfm_run_batches(dense, dense_recs, W)
    rows_recs, _ = _staged_records(groups)
    packers = {}
    for r in rows_recs:                                       # what _ansfm_staged_route does when the engine has the entry
        fm._ansfm_pack_scatter(r, packers)
        assert not any(k in r for k in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "FRAC"))     # the dense arrays are dropped
    assert len(packers) == groups
    rows = _RowsDouble()
    got, _, _ = fm._ansfm_run_batches(rows, rows_recs, W)
    assert len(rows.rows_calls) == groups == len(rows.calls) == len(dense.calls)
    for a, b_ in zip(rows.calls, dense.calls):
        _same_call(a, b_)
    L = dense_recs[0]["lp"].shape[0]
    # one group: state 3 brings two rows; two groups: it leads nothing (states 1, 3 are a group of their own, 1 its first state)
    assert sorted(c["R"] for c in rows.rows_calls) == ([L + 2] if groups == 1 else [L, L + 2])
    assert len(got) == len(want) == 5
    for k in range(5):
        assert np.array_equal(got[k], want[k]) and got[k].shape == (W, 1)
    assert len({g.tobytes() for g in got}) == 5               # five different spectra: none could stand in for another


def test_engine_without_the_rows_entry_keeps_the_dense_call():
    """the staged route packs only `if hasattr(eng, "cirsrad_ck_scatter_batch_rows")`; records that were not packed take the
    dense call whatever the engine offers"""
    fm = _fm()
    recs, W = _staged_records(1)
    eng = _RowsDouble()
    out, _, _ = fm._ansfm_run_batches(eng, recs, W)
    assert len(eng.calls) == 1 and eng.rows_calls == [] and len(out) == 5
    import inspect
    from archnemesis_dist_amd.jacobian_dropin import JacobianGPU
    assert 'hasattr(eng, "cirsrad_ck_scatter_batch_rows")' in inspect.getsource(JacobianGPU._ansfm_staged_route)


@pytest.mark.needs_reference
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")
def test_staged_scattering_jacobian_of_the_reference_case_by_rows(oracle, monkeypatch, golden_dir):
    """jacobian_c4's inputs through the subclass, staged route, twice: an engine double with the dense entry only and one that
    also offers the rows entry (expanding into the same oracle answer).  The rows double receives, expanded, what the dense one
    receives, and YN / KK are the same numbers."""
    import shutil
    import tempfile
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    from oracle import gen_golden_jacobian_ms as gm
    from test_dropin_reference import OracleEngineDouble
    from archnemesis_dist_amd.continuum_rows import expand_rows
    import archnemesis_dist_amd.forward_model as fmod

    class Recording(OracleEngineDouble):
        def cirsrad_ck_scatter_batch(self, ISPACE, lp, lt, am, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac, radg, *rest, **kw):
            self.seen = getattr(self, "seen", []) + [[np.array(a) for a in (lp, lt, am, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac,
                                                                             radg)]]
            return super().cirsrad_ck_scatter_batch(ISPACE, lp, lt, am, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac, radg, *rest, **kw)

    class WithRows(Recording):
        def cirsrad_ck_scatter_batch_rows(self, ISPACE, lp, lt, am, cont_row, cia, dust, ray, sca, phasarr, lfrac_rows, radg, *rest, **kw):
            self.R = getattr(self, "R", []) + [(dust.shape[0], cont_row.shape)]
            return self.cirsrad_ck_scatter_batch(ISPACE, lp, lt, am, *expand_rows(cont_row, cia, dust, ray, sca), phasarr,
                                                 expand_rows(cont_row, lfrac_rows)[0], radg, *rest, **kw)

    ans = import_reference()
    cwd = os.getcwd()
    res = {}
    for cls in (Recording, WithRows):
        work = tempfile.mkdtemp(prefix="ansfm_rows_")
        try:
            gj.setup_c1(ans, work)
            os.chdir(work)
            gj.setup_c1(ans, work, seed=4, case=gm.CASE)
            double = cls(oracle)
            monkeypatch.setattr(fmod, "get_engine", lambda device=0, d=double: d)
            fmod.set_strict(True)
            fm = gj.cut_case(ans, cls=fmod.make_gpu_forward_model(ans.ForwardModel_0), nkeep=gm.NKEEP, free=gm.FREE)
            fm.ansfm_jacobian_route = "staged"
            YN, KK = fm.jacobian_nemesis(NCores=1, analytical_gradient=True)
            assert fm.ansfm_last_jacobian["route"] == "staged"
            res[cls] = (YN, KK, double)
        finally:
            fmod.set_strict(False)
            os.chdir(cwd)
            shutil.rmtree(work, ignore_errors=True)
    (YN0, KK0, d0), (YN1, KK1, d1) = res[Recording], res[WithRows]
    assert not hasattr(d0, "R") and len(d1.R) == len(d1.seen) == len(d0.seen) >= 1
    for a, b_ in zip(d0.seen, d1.seen):
        for x, y in zip(a, b_):
            assert x.shape == y.shape and np.array_equal(x, y)
    n, L = d1.R[0][1]
    assert n == 6 and L <= d1.R[0][0] < n * L                  # fewer rows than (state, layer) pairs
    assert np.array_equal(YN0, YN1) and np.array_equal(KK0, KK1)
    z = np.load(os.path.join(golden_dir, "jacobian_c4.npz"))
    np.testing.assert_allclose(YN1, z["YN"], rtol=5e-7)


# ---- 3. slices of the rows form; the sharded Jacobian ------------------------------------------------------------------------
class _ToyRowsEngine(_ToyEngine):
    """the toy engine's spectrum from the rows form of the same inputs"""

    def cirsrad_ck_scatter_batch_rows(self, **kw):
        from archnemesis_dist_amd.continuum_rows import expand_rows
        W = self.e - self.s
        cont_row = kw.pop("cont_row")
        rows = [kw.pop(k) for k in ROWS]
        n, L = kw["lay_temp"].shape
        assert cont_row.shape == (n, L) and cont_row.max() < rows[1].shape[0]
        for k, a in zip(ROWS, rows):
            assert a is None or a.shape[-1] == W, k           # cut along the rows' wavenumber axis
        kw.update(zip(DENSE, expand_rows(cont_row, *rows)))
        return self.cirsrad_ck_scatter_batch(**kw)


def test_scatter_slice_inputs_cut_the_rows_wavenumber_axis():
    from archnemesis_dist_amd.continuum_rows import rows_kwargs
    from archnemesis_dist_amd.jacobian import scatter_slice_inputs
    z = _toy_inputs(7)
    zr = rows_kwargs(z)
    assert not any(k in zr for k in DENSE) and zr["TAUCIA_rows"] is None and zr["TAURAY_rows"] is None
    R = zr["TAUDUST_rows"].shape[0]
    assert zr["TAUDUST_rows"].shape == (R, 7) and zr["lfrac_rows"].shape == (R, 1, 7) and zr["cont_row"].shape == (4, 3)
    c = scatter_slice_inputs(zr, 2, 5)
    assert c["cont_row"] is zr["cont_row"] and c["phasarr"] is zr["phasarr"] and c["TAUCIA_rows"] is None
    assert np.array_equal(c["TAUDUST_rows"], zr["TAUDUST_rows"][:, 2:5]) and c["TAUDUST_rows"].flags.c_contiguous
    assert np.array_equal(c["lfrac_rows"], zr["lfrac_rows"][:, :, 2:5]) and np.array_equal(c["radg"], z["radg"][:, 2:5])
    assert np.array_equal(c["solar"], z["solar"][2:5])
    YN, KK = None, None
    from archnemesis_dist_amd.jacobian import jacobian_scatter_sharded
    XN = np.array([1.0, 2.0, 0.0])
    YN, KK = jacobian_scatter_sharded(_ToyRowsEngine(7, 0, 7, []), zr, XN, [0, 1, 2])
    YN1, KK1 = jacobian_scatter_sharded(_ToyEngine(7, 0, 7, []), z, XN, [0, 1, 2])
    assert np.array_equal(YN, YN1) and np.array_equal(KK, KK1)


def test_scatter_sharded_rows_gather_gloo(tmp_path):
    """two gloo ranks, each cutting its part of the rows: YN / KK equal the one-rank result of the dense form bit for bit"""
    W, world = 7, 2
    script = textwrap.dedent(f'''
        import os, sys
        sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
        import numpy as np, torch.distributed as dist
        from archnemesis_dist_amd.continuum_rows import rows_kwargs
        from archnemesis_dist_amd.jacobian import jacobian_scatter_sharded, chunk_range
        from test_scatter_wavenumber_shard import _ToyEngine, _toy_inputs
        from test_scatter_rows import _ToyRowsEngine
        dist.init_process_group("gloo")
        rank, world = dist.get_rank(), dist.get_world_size()
        z = _toy_inputs({W})
        XN = np.array([1.0, 2.0, 0.0])
        YN1, KK1 = jacobian_scatter_sharded(_ToyEngine({W}, 0, {W}, []), z, XN, [0, 1, 2])
        s, e = chunk_range({W}, world, rank)
        log = []
        YN, KK = jacobian_scatter_sharded(_ToyRowsEngine({W}, s, e, log), rows_kwargs(z), XN, [0, 1, 2], rank=rank, world_size=world)
        assert log == [e - s], log
        assert YN.shape == (2 * {W},) and KK.shape == (2 * {W}, 3)
        assert np.array_equal(YN, YN1) and np.array_equal(KK, KK1)
        print("rank", rank, "ok")
        dist.destroy_process_group()
    ''')
    f = tmp_path / "swr.py"
    f.write_text(script)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", "29671", str(f)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == world


def test_rows_entry_is_declared_exported_and_bound():
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import _lib
    assert "ansfm_cirsrad_ck_scatter_batch_rows" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "ansfm.h")) as f:
        assert "int ansfm_cirsrad_ck_scatter_batch_rows(" in f.read()
    assert hasattr(pkg.AnsfmEngine, "cirsrad_ck_scatter_batch_rows")


# ---- on the GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    import archnemesis_dist_amd as pkg
    es = [pkg.AnsfmEngine(0) for _ in range(4)]
    yield es
    for e in es:
        e.close()


def _rows(args):
    from archnemesis_dist_amd.continuum_rows import rows_kwargs
    return rows_kwargs(args)


def _both(e, args):
    """the dense entry and the rows entry on the same context -> (dense, its cache count, rows, its cache count)"""
    dense = e.cirsrad_ck_scatter_batch(**args)
    hd = e.last_scatter_cache()
    rows = e.cirsrad_ck_scatter_batch_rows(**_rows(args))
    return dense, hd, rows, e.last_scatter_cache()


def _single(e, args, m):
    at = lambda a: None if a is None else np.asarray(a)[m]
    return e.cirsrad_ck_scatter(args["ISPACE"], args["lay_press_pa"][m], args["lay_temp"][m], args["amount"][m], at(args["TAUCIA"]),
                                at(args["TAUDUST"]), at(args["TAURAY"]), at(args["TAUSCAT"]), args["phasarr"], at(args["lfrac"]),
                                args["radg"][m], args["sol_angs"], args["emiss_angs"], args["aphis"], args["solar"], args["lowbc"],
                                args["brdf_matrix"], args["mu1"], args["wt1"], args["nf"], args["nphi"], args["iray"], args["imie"])


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (8, 2), (16, 4)])       # lane kernels, padded to 16 streams, matrix-core chains
@pytest.mark.parametrize("up,lowbc", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_rows_equal_dense_on_a_ktable(engines, NMU, NF, up, lowbc):
    """W = 241, G = 4, L = 12, one aerosol and Rayleigh, five models: same bits, same layers from the cache"""
    z = _ktable_case(NMU, NF, lowbc)
    W = z["WAVE"].shape[0]
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    args = _batch_args(z, _models(z), up, lowbc, NF)
    assert _rows(args)["TAUDUST_rows"].shape == (12 + 2, W)
    dense, hd, rows, hr = _both(e, args)
    assert rows.shape == dense.shape == (5, W, 2)
    assert np.array_equal(rows, dense)
    assert hr == hd and hr[0] > 0, (hd, hr)
    assert e.last_layer_rows()[0] < 5 * 12


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])
def test_rows_equal_dense_on_an_lbl_table_in_windows(engines, monkeypatch, NMU, NF):
    """G = 1, W = 300 in windows of 64: the slabs are the windows"""
    from test_lbl_scatter import _lbl_inputs
    monkeypatch.setenv("ANSFM_MS_WINDOW", "64")
    rng = np.random.default_rng(7300 + NMU)
    W, L, S = 300, 12, 2
    z = _lbl_inputs(rng, W, L, S, NMU, NF, 1, 1, 1, 1)
    e = engines[0]
    e.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    for up in (False, True):
        args = _batch_args(z, _models(z), up, 1, NF)
        dense = e.cirsrad_ck_scatter_batch(**args)
        hd, wd = e.last_scatter_cache(), e.last_scatter_windows()
        rows = e.cirsrad_ck_scatter_batch_rows(**_rows(args))
        assert np.array_equal(rows, dense)
        assert e.last_scatter_cache() == hd and hd[0] > 0
        assert e.last_scatter_windows() == wd == (5, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 2), (9, 2)])       # (9: the wavefront kernel with ANSFM_MS_PAD16=0)
def test_rows_equal_dense_over_several_slabs(engines, monkeypatch, NMU, NF):
    """a k-table with ANSFM_MS_SLAB=64: four slabs of the axis, the slab's copies of TAURAY and the fractions rewritten per slab
    and per chunk of models (ANSFM_MS_CHUNK=3: two launches of the other models)"""
    monkeypatch.setenv("ANSFM_MS_SLAB", "64")
    monkeypatch.setenv("ANSFM_MS_CHUNK", "3")
    if NMU == 9:
        monkeypatch.setenv("ANSFM_MS_PAD16", "0")
    z = _ktable_case(NMU, NF, 1, seed=3)
    W = z["WAVE"].shape[0]
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    for up in (False, True):
        args = _batch_args(z, _models(z), up, 1, NF)
        dense, hd, rows, hr = _both(e, args)
        assert e.last_scatter_windows() == (4, 64)
        assert np.array_equal(rows, dense) and hr == hd and hr[0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 2)])
def test_rows_equal_dense_without_aerosols_without_cia_one_model_and_model_by_model(engines, monkeypatch, NMU, NF):
    e = engines[0]
    # ncont = 0: Rayleigh alone, no fractions
    from test_gpu_parity import _scatter_inputs
    z0 = _scatter_inputs(np.random.default_rng(7400 + NMU), 241, 4, 12, 3, NMU, NF, 0, 1, 1, 1)
    _ktable_upload(z0)(e, 0, 241)
    a0 = _batch_args(z0, _models(z0), False, 1, NF)
    assert a0["phasarr"].shape[0] == 0 and _rows(a0)["lfrac_rows"] is None
    dense, hd, rows, hr = _both(e, a0)
    assert np.array_equal(rows, dense) and hr == hd
    # TAUCIA = None; then TAURAY = None too (the chains read zeros)
    z = _ktable_case(NMU, NF, 1, seed=4)
    W = z["WAVE"].shape[0]
    _ktable_upload(z)(e, 0, W)
    args = _batch_args(z, _models(z), True, 1, NF)
    for drop in (("TAUCIA",), ("TAUCIA", "TAURAY")):
        a = dict(args, **{k: None for k in drop})
        if "TAURAY" in drop:
            a["iray"] = 0
        dense, hd, rows, hr = _both(e, a)
        assert np.array_equal(rows, dense) and hr == hd and hr[0] > 0
    # n_models = 1
    one = {k: (v[:1] if k in DENSE + ("lay_press_pa", "lay_temp", "amount", "radg") else v) for k, v in args.items()}
    dense, hd, rows, hr = _both(e, one)
    assert rows.shape == (1, W, 2) and np.array_equal(rows, dense) and hr == hd
    # model by model: de-duplication off, and the layer cache switched off
    e.set_layer_dedup(False)
    try:
        dense, hd, rows, hr = _both(e, args)
    finally:
        e.set_layer_dedup(True)
    assert np.array_equal(rows, dense) and hr == hd == (0, 5 * 12)
    cached = e.cirsrad_ck_scatter_batch_rows(**_rows(args))
    assert np.array_equal(cached, rows)
    monkeypatch.setenv("ANSFM_MS_LAYER_CACHE", "0")
    assert np.array_equal(e.cirsrad_ck_scatter_batch_rows(**_rows(args)), dense)
    assert e.last_scatter_cache() == (0, 5 * 12)


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(16, 3), (8, 2), (5, 2)])
@pytest.mark.parametrize("up,lowbc", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_models_that_share_every_layer_with_model_0(engines, NMU, NF, up, lowbc):
    """L = 12 is a multiple of the prefix step: a model identical to model 0 in everything, and one identical in every layer
    with another boundary radiance, start their adding sweep behind the last layer (16 streams).  Every model equals its own
    single-model call bit for bit, through the rows entry and through the dense one."""
    z = _ktable_case(NMU, NF, lowbc, seed=5)
    W = z["WAVE"].shape[0]
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    b = _models(z, n=7)                                        # models 5 and 6 are copies of model 0 ...
    b["radg"][6] *= 1.1                                        # ... 6 with another radg
    args = _batch_args(z, b, up, lowbc, NF)
    zr = _rows(args)
    assert np.array_equal(zr["cont_row"][5], np.arange(12)) and np.array_equal(zr["cont_row"][6], np.arange(12))
    rows = e.cirsrad_ck_scatter_batch_rows(**zr)
    hits = e.last_scatter_cache()
    assert hits[0] >= 2 * 12                                   # at least all layers of models 5 and 6
    dense = e.cirsrad_ck_scatter_batch(**args)
    assert e.last_scatter_cache() == hits
    for m in range(7):
        own = _single(e, args, m)
        assert np.array_equal(rows[m], own), m
        assert np.array_equal(dense[m], own), m
    assert np.array_equal(rows[5], rows[0])
    assert not np.array_equal(rows[6], rows[0])


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 2)])
def test_equal_content_under_two_indices_loses_hits_not_bits(engines, NMU, NF):
    z = _ktable_case(NMU, NF, 1, seed=6)
    W = z["WAVE"].shape[0]
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    args = _batch_args(z, _models(z), False, 1, NF)
    zr = _rows(args)
    one = e.cirsrad_ck_scatter_batch_rows(**zr)
    hits_one = e.last_scatter_cache()
    R, L = zr["TAUDUST_rows"].shape[0], 12
    two = dict(zr)
    for k in ROWS:                                             # model 0's rows once more, behind the others ...
        two[k] = np.concatenate([zr[k], zr[k][:L]], axis=0)
    two["cont_row"] = zr["cont_row"].copy()
    two["cont_row"][2] = R + np.arange(L)                      # ... and model 2 (a gas change: its continuum is model 0's) points there
    got = e.cirsrad_ck_scatter_batch_rows(**two)
    hits_two = e.last_scatter_cache()
    assert np.array_equal(got, one)
    assert hits_two[1] == hits_one[1] and 0 < hits_two[0] < hits_one[0], (hits_one, hits_two)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["ktable", "lbl"])
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 2)])
def test_rows_slices_side_by_side_equal_the_whole_axis(engines, monkeypatch, table, NMU, NF):
    from archnemesis_dist_amd.jacobian import chunk_range, scatter_slice_inputs
    if table == "lbl":
        from test_lbl_scatter import _lbl_inputs
        monkeypatch.setenv("ANSFM_MS_WINDOW", "64")
        z = _lbl_inputs(np.random.default_rng(7500 + NMU), 300, 12, 2, NMU, NF, 1, 1, 1, 1)
        upload = lambda e, s, t: e.upload_lbltable(np.ascontiguousarray(z["K"][s:t]), z["TPRESS"], z["TTEMP"], z["WAVE"][s:t])
    else:
        z = _ktable_case(NMU, NF, 1, seed=7)
        upload = _ktable_upload(z)
    W = z["WAVE"].shape[0]
    args = _batch_args(z, _models(z), False, 1, NF)
    zr = _rows(args)
    upload(engines[0], 0, W)
    whole = engines[0].cirsrad_ck_scatter_batch(**args)
    hits = engines[0].last_scatter_cache()
    assert np.array_equal(engines[0].cirsrad_ck_scatter_batch_rows(**zr, wave_slice=(0, W)), whole)
    parts = []
    for r, e in enumerate(engines[1:]):
        s, t = chunk_range(W, 3, r)
        upload(e, s, t)
        cut = scatter_slice_inputs(zr, s, t)
        assert cut["TAUDUST_rows"].shape[1] == t - s
        parts.append(e.cirsrad_ck_scatter_batch_rows(**cut, wave_slice=(s, W)))
        assert e.last_scatter_cache() == hits
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


@pytest.mark.gpu
def test_bad_row_indices_are_refused_and_the_context_goes_on(engines):
    z = _ktable_case(16, 2, 1, seed=8)
    W = z["WAVE"].shape[0]
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    args = _batch_args(z, _models(z), False, 1, 2)
    zr = _rows(args)
    good = e.cirsrad_ck_scatter_batch(**args)
    R = zr["TAUDUST_rows"].shape[0]
    for bad in (-1, R):
        cr = zr["cont_row"].copy()
        cr[3, 7] = bad
        with pytest.raises(ValueError, match="INVALID"):
            e.cirsrad_ck_scatter_batch_rows(**dict(zr, cont_row=cr))
        assert np.array_equal(e.cirsrad_ck_scatter_batch_rows(**zr), good)
    with pytest.raises(ValueError):                            # shape checks before the call
        e.cirsrad_ck_scatter_batch_rows(**dict(zr, cont_row=zr["cont_row"][:, :-1]))
    with pytest.raises(ValueError):
        e.cirsrad_ck_scatter_batch_rows(**dict(zr, TAUDUST_rows=zr["TAUDUST_rows"][:, :-1]))
    with pytest.raises(ValueError):
        e.cirsrad_ck_scatter_batch_rows(**dict(zr, lfrac_rows=zr["lfrac_rows"][:-1]))
    with pytest.raises(ValueError):
        e.cirsrad_ck_scatter_batch_rows(**dict(zr, cont_row=zr["cont_row"].astype(float)))
