"""Shared by the single-scattering batch tests: synthetic Jacobian-like states for ansfm_cirsrad_ck_singlescatt_batch, the
reference's recipe on the oracle's pieces, and the fixture's KK check."""
import numpy as np


def synthetic_table(kind, W, G, S, NP=8, NT=6, seed=31):
    """kind: "sorted" (k-table, monotone in g), "scrambled" (its g axis permuted: the generic merge), "lbl" (G = 1).
    -> dict(K, PRESS, TEMP, WAVE, delg)"""
    from archnemesis_dist_amd import synthetic as syn
    WAVE = 2000.0 + 3.0 * np.arange(W)
    if kind == "lbl":
        rng = np.random.default_rng(seed)
        PRESS = np.logspace(-6, 1.2, NP); TEMP = np.linspace(90.0, 320.0, NT)
        K = (10.0 ** rng.uniform(-24, -20.5, (W, 1, 1, S))) * PRESS[None, :, None, None] ** 0.15 * (TEMP[None, None, :, None] / 150.0) ** 0.8
        return dict(K=K, PRESS=PRESS, TEMP=TEMP, WAVE=WAVE, delg=np.ones(1))
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=seed)
    if kind == "scrambled":
        K = np.ascontiguousarray(K[:, np.random.default_rng(5).permutation(G)])
    _, delg = syn.gauss_legendre_01(G)
    return dict(K=K, PRESS=PRESS, TEMP=TEMP, WAVE=WAVE, delg=delg)


def upload(eng, t):
    if t["K"].ndim == 4:
        eng.upload_lbltable(t["K"], t["PRESS"], t["TEMP"], t["WAVE"])
    else:
        eng.upload_ktable(t["K"], t["PRESS"], t["TEMP"], t["WAVE"], t["delg"])


def base_state(W, S, L, seed=88, omega_scale=1.0):
    """One state as tests/test_gpu_parity.py::_singlescatt_vs_oracle builds it: two paths of different length and geometry,
    a layer without aerosol, BRDF > 0; the scattering opacity raised so that the albedo reaches about 0.9."""
    rng = np.random.default_rng(seed)
    lp = np.logspace(5.0, 1.0, L); lt = np.linspace(230.0, 150.0, L)
    am = 10.0 ** rng.uniform(17, 19.5, (S, L)) * (lp[None, :] / lp[0])
    TAURAY = 10.0 ** rng.uniform(-4, -2, (W, L)); TAUSCAT = omega_scale * 10.0 ** rng.uniform(-3, -1, (W, L)); TAUSCAT[:, 4] = 0.0
    TAUDUST = TAUSCAT * 1.1; TAUCIA = 10.0 ** rng.uniform(-5, -3, (W, L))
    P = 2
    phase = 10.0 ** rng.uniform(-1.5, 0.3, (P, W, L))
    LAYINC = np.zeros((L, P), dtype=np.int32)
    LAYINC[:, 0] = np.arange(L - 1, -1, -1); LAYINC[:L - 2, 1] = np.arange(L - 1, 1, -1)
    NLAYIN = np.array([L, L - 2], dtype=np.int32)
    sol = np.array([30.0, 55.0]); emi = np.array([10.0, 40.0])
    SCALE = np.where(np.arange(L)[:, None] < NLAYIN[None, :], 1.0 / np.cos(np.deg2rad(emi))[None, :], 0.0)
    return dict(lp=lp, lt=lt, am=am, cont=TAUCIA + TAUDUST + TAURAY, sca=TAURAY + TAUSCAT, phase=phase, LAYINC=LAYINC, NLAYIN=NLAYIN,
                sol=sol, emi=emi, SCALE=SCALE, EMIS=rng.uniform(0.7, 1.0, W), BRDF=rng.uniform(0.02, 0.15, (W, P)),
                SOLF=10.0 ** rng.uniform(-8, -7, W), xfac=rng.uniform(0.5, 2.0, W))


def emtemp_of(b, lt):
    L = lt.shape[-1]
    return np.where(np.arange(L)[:, None] < b["NLAYIN"][None, :], lt[b["LAYINC"]], 0.0)


def jacobian_like_states(b, tsurf0, tsurf_other):
    """State 0 and six more that differ from it in, in this order: one layer's temperature, one gas amount, one layer's
    scattering opacity, one path's phase function only, TSURF only, nothing.  -> dict of arrays with a leading model axis."""
    n = 7
    rep = lambda a: np.repeat(np.asarray(a)[None], n, axis=0).copy()
    lp, lt, am, cont, sca, phase = rep(b["lp"]), rep(b["lt"]), rep(b["am"]), rep(b["cont"]), rep(b["sca"]), rep(b["phase"])
    L = lp.shape[1]
    lt[1, L // 3] *= 1.01
    am[2, 1, L // 2] *= 1.05
    sca[3, :, (2 * L) // 3] *= 1.1
    phase[4, 1, :, L - 3] *= 1.2                 # path 1 only: path 0 of this state is state 0's to the ground
    TSURF = np.full(n, float(tsurf0)); TSURF[5] = tsurf_other
    EMTEMP = np.stack([emtemp_of(b, lt[m]) for m in range(n)])
    return dict(lp=lp, lt=lt, am=am, cont=cont, sca=sca, phase=phase, SCALE=rep(b["SCALE"]), EMTEMP=EMTEMP, TSURF=TSURF)


def batch_call(eng, b, s, ispace=0, sel=slice(None)):
    return eng.cirsrad_ck_singlescatt_batch(ispace, s["lp"][sel], s["lt"][sel], s["am"][sel], s["cont"][sel], s["sca"][sel], s["phase"][sel],
                                            b["NLAYIN"], b["LAYINC"], s["SCALE"][sel], s["EMTEMP"][sel], s["TSURF"][sel], b["EMIS"],
                                            b["BRDF"], b["SOLF"], b["sol"], b["emi"], xfac=b["xfac"])


def single_call(eng, b, s, m, ispace=0):
    return eng.cirsrad_ck_singlescatt(ispace, s["lp"][m], s["lt"][m], s["am"][m], s["cont"][m], s["sca"][m], s["phase"][m], b["NLAYIN"],
                                      b["LAYINC"], s["SCALE"][m], s["EMTEMP"][m], float(s["TSURF"][m]), b["EMIS"], b["BRDF"], b["SOLF"],
                                      b["sol"], b["emi"], xfac=b["xfac"])


def oracle_chain(orc, t, ispace, lp, lt, am, cont, sca, phase, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMIS, BRDF, SOLF, sol, emi, xfac=None):
    """The reference's recipe for one state on the oracle's pieces: calc_k + k_overlap, TAUTOT (:3989), OMEGA (:4276-4283),
    LAYINC x SCALE (:4006), calc_singlescatt_plane_spectrum per path, xfac, g-quadrature (:4504) -> SPECOUT (NWAVE, NPATH)."""
    k = orc.calc_k(t["K"], t["PRESS"], t["TEMP"], np.asarray(lp) / 101325.0, lt)
    tautot = orc.k_overlap(t["delg"], k, am) + np.asarray(cont)[:, None, :]
    omega = np.where(tautot > 0, np.asarray(sca)[:, None, :] / np.where(tautot > 0, tautot, 1.0), 0.0)
    W, P = len(t["WAVE"]), len(np.atleast_1d(sol))
    xf = np.ones(W) if xfac is None else np.asarray(xfac)
    out = np.zeros((W, P))
    for ip in range(P):
        n = int(NLAYIN[ip]); li = np.asarray(LAYINC)[:n, ip]
        sp = orc.calc_singlescatt_plane_spectrum(ispace, t["WAVE"], tautot[:, :, li] * np.asarray(SCALE)[:n, ip], np.asarray(EMTEMP)[:n, ip],
                                                 omega[:, :, li], np.asarray(phase)[ip][:, li], TSURF, EMIS, np.asarray(BRDF)[:, ip], SOLF,
                                                 np.atleast_1d(sol)[ip], np.atleast_1d(emi)[ip])
        out[:, ip] = np.tensordot(sp * xf[:, None], np.asarray(t["delg"], dtype=float), axes=([1], [0]))
    return out


def fixture_table(z):
    return dict(K=z["K"], PRESS=z["TPRESS"], TEMP=z["TTEMP"], WAVE=z["WAVE"], delg=z["DELG"])


def fixture_batch_args(z):
    """jacobian_ss.npz -> the positional arguments of cirsrad_ck_singlescatt_batch"""
    n = z["LAY_PRESS"].shape[0]
    amount = np.ascontiguousarray(np.transpose(z["LAY_AMOUNT"], (0, 2, 1))) * 1.0e-4
    return (int(z["ISPACE"]), z["LAY_PRESS"], z["LAY_TEMP"], amount, z["TAUCONT"], z["TAUSCA"], z["PHASE"], z["NLAYIN"], z["LAYINC"],
            z["SCALE"], z["EMTEMP"], np.full(n, float(z["TSURF"])), z["EMISSIVITY"], z["BRDF"], z["SOLFLUX"], z["SOL_ANG"], z["EMISS_ANG"])


def kk_from_spectra(z, SPECOUT):
    """Measurement vectors and KK from per-state spectra (nfm, NWAVE, 1) the reference's way: conv with FWHM = 0 is a linear
    interpolation onto VCONV, then the quotient of :2348-2359 (archnemesis_dist_amd.jacobian.finite_difference_jacobian)."""
    from archnemesis_dist_amd.jacobian import finite_difference_jacobian
    Y = np.stack([np.interp(z["VCONV"], z["WAVE"], s[:, 0]) for s in SPECOUT], axis=1)
    return finite_difference_jacobian(Y, z["XN"], z["inum"], iYN=0, FIX=z["FIX"])


def assert_kk(KK, z, tol=1e-4):
    """Every free column within tol of that column's largest element in the reference's KK (the project's contract); the
    fixed columns stay zero.  The figures are printed before they are asserted."""
    worst = {}
    for ix in z["inum"]:
        scale = np.abs(z["KK"][:, ix]).max()
        assert scale > 0
        worst[int(ix)] = float(np.abs(KK[:, ix] - z["KK"][:, ix]).max() / scale)
    print("KK column errors / column maximum:", {k: "%.2e" % v for k, v in worst.items()})
    assert max(worst.values()) <= tol, worst
    fixed = np.setdiff1d(np.arange(KK.shape[1]), z["inum"])
    assert not KK[:, fixed].any()
