"""The scattering Jacobian sharded along the spectral axis: ansfm_cirsrad_ck_scatter_batch_slice (engine:
cirsrad_ck_scatter_batch(wave_slice=...)) and jacobian.jacobian_scatter_sharded.  Every rank walks the Hansen factors over the
whole axis and keeps those of its slice, so the parts side by side must equal the call over the whole axis bit for bit."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- without the GPU: host slicing and the gather's ordering -------------------------------------------------------------------
class _ToyEngine:
    """cirsrad_ck_scatter_batch on a slice: a spectrum built from the sliced inputs, so that a wrong cut or a wrong ordering
    of the gathered parts shows in the result"""

    def __init__(self, W_full, s, e, log):
        self.W_full, self.s, self.e, self.log = W_full, s, e, log

    def cirsrad_ck_scatter_batch(self, **kw):
        w_begin, W_full = kw.pop("wave_slice")
        assert (w_begin, W_full) == (self.s, self.W_full)
        W = self.e - self.s
        assert kw["phasarr"].shape[1] == W_full                              # the walk needs the whole axis
        for k in ("TAUDUST", "TAUSCAT", "radg", "lfrac"):
            assert kw[k].shape[1] == W, k
        assert kw["solar"].shape == (W,) and kw["brdf_matrix"].shape[0] == W and kw["TAURAY"] is None
        P = len(kw["sol_angs"])
        self.log.append(W)
        return (kw["radg"][:, :, :1] * (1.0 + np.arange(P))[None, None, :] + kw["TAUDUST"][:, :, 1:2] * kw["lay_temp"][:, None, :1]
                + kw["solar"][None, :, None])


def _toy_inputs(W, n=4, P=2, L=3, NMU=2, seed=3):
    rng = np.random.default_rng(seed)
    return dict(ISPACE=0, lay_press_pa=np.tile(np.logspace(5, 2, L), (n, 1)), lay_temp=rng.uniform(100, 200, (n, L)),
                amount=np.ones((n, 2, L)), TAUCIA=None, TAUDUST=rng.uniform(0, 1, (n, W, L)), TAURAY=None,
                TAUSCAT=rng.uniform(0, 1, (n, W, L)), phasarr=np.zeros((1, W, 2, 5)), lfrac=np.ones((n, W, 1, L)),
                radg=rng.uniform(1, 2, (n, W, NMU)), sol_angs=[30.0] * P, emiss_angs=[20.0] * P, aphis=[0.0] * P,
                solar=rng.uniform(0, 1, W), lowbc=0, brdf_matrix=np.zeros((W, NMU, NMU, 2)), mu1=np.ones(NMU), wt1=np.ones(NMU),
                nf=1, nphi=11, iray=0, imie=0)


def test_scatter_slice_inputs_cut_the_wavenumber_axis_only():
    from archnemesis_dist_amd.jacobian import scatter_slice_inputs
    z = _toy_inputs(7)
    c = scatter_slice_inputs(z, 2, 5)
    assert c["TAUDUST"].shape == (4, 3, 3) and np.array_equal(c["TAUDUST"], z["TAUDUST"][:, 2:5])
    assert np.array_equal(c["radg"], z["radg"][:, 2:5]) and np.array_equal(c["lfrac"], z["lfrac"][:, 2:5])
    assert np.array_equal(c["solar"], z["solar"][2:5]) and c["brdf_matrix"].shape == (3, 2, 2, 2)
    assert c["phasarr"] is z["phasarr"] and c["lay_temp"] is z["lay_temp"] and c["TAURAY"] is None


def test_scatter_sharded_one_rank_orders_rows_path_major():
    from archnemesis_dist_amd.jacobian import jacobian_scatter_sharded
    z = _toy_inputs(5)
    spec = _ToyEngine(5, 0, 5, []).cirsrad_ck_scatter_batch(**z, wave_slice=(0, 5))      # (n, W, P)
    XN = np.array([1.0, 2.0, 0.0])
    YN, KK = jacobian_scatter_sharded(_ToyEngine(5, 0, 5, []), z, XN, [0, 1, 2])
    Y = np.transpose(spec, (0, 2, 1)).reshape(4, -1)                        # path outer, wavenumber inner
    assert np.array_equal(YN, Y[0])
    den = np.array([0.05, 0.1, 0.05])
    np.testing.assert_allclose(KK, ((Y[1:] - Y[0]) / den[:, None]).T, rtol=1e-13, atol=0)


@pytest.mark.parametrize("W,world", [(7, 3), (2, 3)])            # ragged parts; more ranks than wavenumbers
def test_scatter_sharded_gather_gloo(tmp_path, W, world):
    """Each rank cuts its part of the axis, the toy engine sees only that part, and the gathered YN / KK equal the one-rank
    result bit for bit, NPATH = 2; a rank without wavenumbers calls nothing and joins the gather."""
    script = textwrap.dedent(f'''
        import os, sys
        sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
        import numpy as np, torch.distributed as dist
        from archnemesis_dist_amd.jacobian import jacobian_scatter_sharded, chunk_range
        from test_scatter_wavenumber_shard import _ToyEngine, _toy_inputs
        dist.init_process_group("gloo")
        rank, world = dist.get_rank(), dist.get_world_size()
        z = _toy_inputs({W})
        XN = np.array([1.0, 2.0, 0.0])
        YN1, KK1 = jacobian_scatter_sharded(_ToyEngine({W}, 0, {W}, []), z, XN, [0, 1, 2])
        s, e = chunk_range({W}, world, rank)
        log = []
        YN, KK = jacobian_scatter_sharded(_ToyEngine({W}, s, e, log), z, XN, [0, 1, 2], rank=rank, world_size=world)
        assert log == ([e - s] if e > s else []), log
        assert YN.shape == (2 * {W},) and KK.shape == (2 * {W}, 3)
        assert np.array_equal(YN, YN1) and np.array_equal(KK, KK1)
        print("rank", rank, "ok")
        dist.destroy_process_group()
    ''')
    f = tmp_path / "sw.py"
    f.write_text(script)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(29640 + W), str(f)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == world


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
def _models(z, n=5):
    """model 0 and four Jacobian columns: one layer's temperature, one gas amount in three layers, the dust opacity of two
    layers, the surface temperature (the lower boundary radiance and the bottom layer).  Every model differs from model 0 in
    some layer: a model that shares all of them starts its sweep at the top of the stack (lstart == L), a case kept out of
    these batches."""
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0).copy()
    b = dict(lay_press_pa=rep(z["lay_p"]), lay_temp=rep(z["lay_t"]), amount=rep(z["amount"]), TAUCIA=rep(z["TAUCIA"]),
             TAUDUST=rep(z["TAUDUST"]), TAURAY=rep(z["TAURAY"]), TAUSCAT=rep(z["TAUSCAT"]), lfrac=rep(z["lfrac"]), radg=rep(z["radg"]))
    b["lay_temp"][1, 4] *= 1.05
    b["amount"][2, 1, 6:9] *= 1.05
    b["TAUDUST"][3, :, 5:7] *= 1.05
    b["radg"][4] *= 1.1; b["lay_temp"][4, 0] *= 1.02
    return b


def _batch_args(z, b, up, lowbc, NF, iray=1, imie=1):
    sol = np.array([30.0, 120.0]); emi = np.array([160.0, 130.0]) if up else np.array([20.0, 50.0]); azi = np.array([45.0, 0.0])
    return dict(ISPACE=0, **b, phasarr=z["phasarr"], sol_angs=sol, emiss_angs=emi, aphis=azi, solar=z["solar"], lowbc=lowbc,
                brdf_matrix=z["brdf"], mu1=z["MU"], wt1=z["WT"], nf=NF, nphi=101, iray=iray, imie=imie)


def _parts(engines, upload, z, args, W):
    """the batch on each context's slice chunk_range(W, len(engines), r) -> the parts side by side, and each part's cache count"""
    from archnemesis_dist_amd.jacobian import chunk_range, scatter_slice_inputs
    out, hits = [], []
    for r, e in enumerate(engines):
        s, t = chunk_range(W, len(engines), r)
        upload(e, s, t)
        out.append(e.cirsrad_ck_scatter_batch(**scatter_slice_inputs(args, s, t), wave_slice=(s, W)))
        hits.append(e.last_scatter_cache())
    return np.concatenate(out, axis=1), hits


@pytest.fixture(scope="module")
def engines():
    import archnemesis_dist_amd as pkg
    es = [pkg.AnsfmEngine(0) for _ in range(4)]
    yield es
    for e in es:
        e.close()


def _ktable_case(NMU, NF, lowbc, W=241, G=4, L=12, S=3, seed=0):
    from test_gpu_parity import _scatter_inputs
    rng = np.random.default_rng(5100 + NMU + 7 * NF + 11 * lowbc + seed)
    return _scatter_inputs(rng, W, G, L, S, NMU, NF, 1, 1, 1, lowbc)


def _ktable_upload(z):
    return lambda e, s, t: e.upload_ktable(np.ascontiguousarray(z["K"][s:t]), z["TPRESS"], z["TTEMP"], z["WAVE"][s:t], z["DELG"])


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 4), (8, 2)])       # lane kernels, matrix-core chains, padded to 16 streams
@pytest.mark.parametrize("up,lowbc", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_slices_side_by_side_equal_the_whole_axis(engines, NMU, NF, up, lowbc):
    """W = 241, G = 4, L = 12, one aerosol and Rayleigh, five models: three contexts holding chunk_range(241, 3, r) of the
    k-table give, side by side, the call over the whole axis bit for bit, with the same layers taken from the cache."""
    z = _ktable_case(NMU, NF, lowbc)
    W = z["WAVE"].shape[0]
    args = _batch_args(z, _models(z), up, lowbc, NF)
    whole_eng, parts_eng = engines[0], engines[1:]
    _ktable_upload(z)(whole_eng, 0, W)
    whole = whole_eng.cirsrad_ck_scatter_batch(**args)
    hits_whole = whole_eng.last_scatter_cache()
    got, hits = _parts(parts_eng, _ktable_upload(z), z, args, W)
    assert got.shape == whole.shape
    assert np.array_equal(got, whole)
    assert hits_whole[0] > 0 and all(h == hits_whole for h in hits), (hits_whole, hits)


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])
def test_lbl_slices_start_inside_windows(engines, monkeypatch, NMU, NF):
    """G = 1 (LBL table), W = 300 in windows of 64: the slices start at 100 and 200, inside windows of the whole call; each
    rank walks the wavenumbers in front of its slice in carry-only windows.  Parts equal the whole bit for bit."""
    from test_lbl_scatter import _lbl_inputs
    monkeypatch.setenv("ANSFM_MS_WINDOW", "64")
    rng = np.random.default_rng(5300 + NMU)
    W, L, S = 300, 12, 2
    z = _lbl_inputs(rng, W, L, S, NMU, NF, 1, 1, 1, 1)
    args = _batch_args(z, _models(z), False, 1, NF)
    upload = lambda e, s, t: e.upload_lbltable(np.ascontiguousarray(z["K"][s:t]), z["TPRESS"], z["TTEMP"], z["WAVE"][s:t])
    upload(engines[0], 0, W)
    whole = engines[0].cirsrad_ck_scatter_batch(**args)
    assert engines[0].last_scatter_windows() == (5, 64)
    got, hits = _parts(engines[1:], upload, z, args, W)
    assert np.array_equal(got, whole)
    assert all(h == engines[0].last_scatter_cache() for h in hits)


@pytest.mark.gpu
def test_degenerate_and_invalid_slices(engines):
    """w_begin = 0 over the whole axis is the unsliced call; a last slice of one wavenumber works; a slice that does not fit
    the axis is INVALID; a slice without the layer cache is UNSUPPORTED."""
    z = _ktable_case(16, 2, 1, seed=1)
    W = z["WAVE"].shape[0]
    args = _batch_args(z, _models(z), False, 1, 2)
    e = engines[0]
    _ktable_upload(z)(e, 0, W)
    whole = e.cirsrad_ck_scatter_batch(**args)
    assert np.array_equal(e.cirsrad_ck_scatter_batch(**args, wave_slice=(0, W)), whole)
    from archnemesis_dist_amd.jacobian import scatter_slice_inputs
    last = engines[1]
    _ktable_upload(z)(last, W - 1, W)
    one = last.cirsrad_ck_scatter_batch(**scatter_slice_inputs(args, W - 1, W), wave_slice=(W - 1, W))
    assert one.shape == (5, 1, 2) and np.array_equal(one, whole[:, W - 1:])
    _ktable_upload(z)(last, 0, 81)
    cut = scatter_slice_inputs(args, 0, 81)                                  # 81 wavenumbers, placed where they do not fit
    for bad in ((200, W), (-1, W)):
        with pytest.raises(ValueError, match="INVALID"):
            last.cirsrad_ck_scatter_batch(**cut, wave_slice=bad)
    last.set_layer_dedup(False)
    try:
        with pytest.raises(NotImplementedError, match="UNSUPPORTED"):
            last.cirsrad_ck_scatter_batch(**scatter_slice_inputs(args, 0, 81), wave_slice=(0, W))
    finally:
        last.set_layer_dedup(True)


@pytest.mark.gpu
def test_scatter_sharded_jacobian_two_ranks_gloo(tmp_path):
    """torch.distributed.run with two ranks, gloo, both on GPU 0: each rank holds half of the k-table and runs every model on
    it; YN and KK equal the one-rank result bit for bit."""
    script = textwrap.dedent(f'''
        import os, sys
        sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
        import numpy as np, torch.distributed as dist
        import archnemesis_dist_amd as pkg
        from archnemesis_dist_amd.jacobian import jacobian_scatter_sharded, chunk_range
        from test_scatter_wavenumber_shard import _ktable_case, _ktable_upload, _batch_args, _models
        dist.init_process_group("gloo")
        rank, world = dist.get_rank(), dist.get_world_size()
        z = _ktable_case(16, 2, 1, seed=2)
        W = z["WAVE"].shape[0]
        args = _batch_args(z, _models(z), False, 1, 2)
        XN = np.array([150.0, 0.3, 0.02, 0.0])
        one = pkg.AnsfmEngine(0)
        _ktable_upload(z)(one, 0, W)
        YN1, KK1 = jacobian_scatter_sharded(one, args, XN, [0, 1, 2, 3])
        one.close()
        eng = pkg.AnsfmEngine(0)
        s, e = chunk_range(W, world, rank)
        _ktable_upload(z)(eng, s, e)
        YN, KK = jacobian_scatter_sharded(eng, args, XN, [0, 1, 2, 3], rank=rank, world_size=world)
        eng.close()
        assert YN.shape == (2 * W,) and KK.shape == (2 * W, 4)
        assert np.array_equal(YN, YN1) and np.array_equal(KK, KK1)
        assert np.all(np.any(KK != 0, axis=0))
        print("rank", rank, "ok")
        dist.destroy_process_group()
    ''')
    f = tmp_path / "sj.py"
    f.write_text(script)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29651", str(f)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2
