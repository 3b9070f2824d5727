#!/usr/bin/env python
"""Secondary timings on one MI355X (not the driver's bench contract): analytic-gradient CIRSrad at C2,
the multiple-scattering core on a C4-like stack, runtime line-by-line on a reduced C5, batched layering.
Host-pointer entry points: PCIe staging is included in the wall times (noted per line)."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn


def timeit(f, n=3):
    f(); ts = []
    for _ in range(n):
        t = time.perf_counter(); f(); ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None       # "grad" | "ms" | "lbl" | "lblrt" | "layer" | "ss" | "ss_cont"
    eng = pkg.AnsfmEngine(0)
    out = {}
    rng = np.random.default_rng(0)
    if only in (None, "grad"):
        bench_grad(eng, out)
    if only in (None, "ms"):
        bench_ms(eng, out, rng)
    if only in (None, "lbl"):
        bench_lbl(eng, out, rng)
    if only == "lbl_c5":
        bench_lbl(eng, out, rng, full=True)
    if only == "lbl_pc":                                    # C5 size: 400 MB of opacities per host array, on request only
        bench_lbl_pc(eng, out)
    if only == "lblrt":                                     # C5 size: 400 MB of opacities per state, on request only
        bench_lblrt(eng, out)
    if only in (None, "layer"):
        bench_layer(eng, out)
    if only in (None, "maps"):
        bench_maps(eng, out, rng)
    if only in (None, "next"):
        bench_next(eng, out, rng)
    if only == "mie":
        bench_mie(eng, out)
    if only == "brdf":                                      # 0.18 GB of matrix back over PCIe: on request only
        bench_brdf(eng, out)
    if only == "transit":                                   # 1.6 GB dSPECOUT on the host for the un-collapsed route: on request only
        bench_transit(eng, out)
    if only == "so":                                        # 0.33 GB dSPECOUT on the host for the un-collapsed route: on request only
        bench_so(eng, out)
    if only == "limb":                                      # 0.33 GB dSPECOUT on the device for the un-collapsed route: on request only
        bench_limb(eng, out)
    if only == "disc":                                      # NAV dSPECOUT arrays on the host for today's route: on request only
        bench_disc(eng, out)
    if only == "ss":                                        # 10 GB of host arrays: on request only
        bench_ss(eng, out, rng)
    if only == "cia":                                       # 1.6 GB continuum array of the dense route: on request only
        bench_cia(eng, out)
    if only == "grad_cont":                                 # 0.1 GB dTAUCON assembled on the host for the route it replaces: on request only
        bench_grad_cont(eng, out)
    if only == "ss_cont":                                   # 5 GB of host arrays in the array-level route: on request only
        bench_ss_cont(eng, out, rng)
    if only == "scatter_cont":                              # 13 GB of host arrays in the by-hand route: on request only
        bench_scatter_cont(eng, out)
    if only == "phase":                                     # 131 MB of phase functions per population on the host: on request only
        bench_phase(eng, out, rng)
    if only == "ms_phase":                                  # 0.3 GB of phase functions on the host, tens of GB of variants on the device
        bench_ms_phase(eng, out)
    print(json.dumps(out, indent=1))


def calc_phase_host(imie, SWAVE, THETA_TAB, tab, theta, WAVE):
    """Scatter_0.calc_phase restated in NumPy (the host route the GPU entries replace): phase1 on the aerosol grid, then
    interp1d's linear rule along the wavenumbers -> (W, nth, NDUST)"""
    def lin(x, y, xn):
        hi = np.clip(np.searchsorted(x, xn, "left"), 1, len(x) - 1); lo = hi - 1
        ex = (slice(None),) + (None,) * (y.ndim - 1)
        return ((y[hi] - y[lo]) / (x[hi] - x[lo])[ex]) * (xn - x[lo])[ex] + y[lo]
    c = np.cos(theta / 180. * np.pi)
    if imie == 0:
        F, G1, G2 = (a[:, None, :] for a in tab)
        cx = c[None, :, None]
        t1 = (1. - G1 ** 2.) / (1. - 2. * G1 * cx + G1 ** 2.) ** 1.5
        t2 = (1. - G2 ** 2.) / (1. - 2. * G2 * cx + G2 ** 2.) ** 1.5
        phase1 = (F * t1 + (1.0 - F) * t2) / (4.0 * np.pi)
    elif imie == 1:
        phase1 = np.moveaxis(lin(THETA_TAB, np.moveaxis(tab, 1, 0), theta), 0, 1)
    else:
        phase1 = np.zeros((tab.shape[0], theta.size, tab.shape[2]))
        p0, p1 = np.ones_like(c), c
        for l in range(tab.shape[1]):
            pl = p0 if l == 0 else p1
            if l >= 2:
                pl = ((2 * l - 1) * c * p1 - (l - 1) * p0) / l
                p0, p1 = p1, pl
            phase1 += pl[None, :, None] * tab[:, l, None, :]
    return lin(SWAVE, phase1, WAVE)


def bench_phase(eng, out, rng, n=5):
    """The aerosol phase function on the calculation grid (41 angles, 2 populations), host route against device route:
      (a) ansfm_calc_phase per IMIE at W = 1e4 and 2e5: kernel time, end to end with the result copied back, beside the NumPy
          restatement of Scatter_0.calc_phase on the host;
      (b) the multiple-scattering batch: cirsrad_ck_scatter_batch_cont with PHASE_ARRAY formed on the host for every call
          (calc_phase + staging, the parent's route) against cirsrad_ck_scatter_batch_src, 5 streams / NF 2, at C4 size (W = 1e4,
          G = 20) and on an LBL window (W = 2e5, G = 1), `states` forward models of 100 layers;
      (c) the same pair for the single-scattering batch (phase_fn at one path's angle) at W = 1e4, 201 states.
    Medians of n runs after a warm-up.
        python tools/bench_extra.py phase [a|b|c|all] [states of (b)] [W of the LBL window]"""
    import torch
    from bench import torch_ktable
    from archnemesis_dist_amd.jacobian import perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel, BatchedCKSingleScatterModel
    part = sys.argv[2] if len(sys.argv) > 2 else "all"
    states_b = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    W_lbl = int(sys.argv[4]) if len(sys.argv) > 4 else 200000
    ND, NWS, S, L, NP, NT = 2, 12, 8, 100, 20, 15
    TH = np.linspace(0.0, 180.0, 41)
    res = {"angles": 41, "populations": ND, "median_of": n}

    def tables(imie, SWAVE):
        x = np.linspace(0.0, 1.0, NWS)[:, None] + 0.1 * np.arange(ND)[None]
        g = 0.3 + 0.5 * x / 1.1
        if imie == 0:
            return np.array([0.5 + 0.3 * x / 1.1, g, -0.2 - 0.2 * x / 1.1])
        if imie == 1:
            c = np.cos(np.deg2rad(TH))[None, :, None]
            return (1 - g[:, None] ** 2) / (1 + g[:, None] ** 2 - 2 * g[:, None] * c) ** 1.5 / (4 * np.pi)
        l = np.arange(36)[None, :, None]
        return (2 * l + 1) * g[:, None] ** l / (4 * np.pi)

    def grid(W):
        WAVE = 200.0 + (1000.0 / W) * np.arange(W)
        return WAVE, np.linspace(0.9 * WAVE[0], 1.1 * WAVE[-1], NWS)

    def phasarr_host(imie, SWAVE, tab, WAVE):
        """ForwardModel_0.py:5128-5142 on the host"""
        arr = np.zeros((ND, WAVE.size, 2, TH.size))
        if imie == 0:
            for d in range(ND):
                for k, slot in ((0, -1), (1, -2), (2, -3)):
                    arr[d, :, 0, slot] = np.interp(WAVE, SWAVE, tab[k][:, d])
        else:
            arr[:, :, 0, :] = np.transpose(calc_phase_host(imie, SWAVE, TH, tab, TH, WAVE), (2, 0, 1))
        arr[:, :, 1, :] = np.cos(TH * np.pi / 180)
        return np.ascontiguousarray(arr[:, :, :, ::-1])

    if part in ("a", "all"):
        for W in (10000, 200000):
            WAVE, SWAVE = grid(W)
            for imie in (0, 1, 2):
                tab = np.ascontiguousarray(tables(imie, SWAVE))
                run = lambda: eng.calc_phase(imie, SWAVE, TH, tab, TH, WAVE)
                got = run()
                host = calc_phase_host(imie, SWAVE, TH, tab, TH, WAVE)
                res["calc_phase_imie%d_W%d" % (imie, W)] = {
                    "gpu_end_to_end_s": timeit(run, n), "gpu_kernel_ms": eng.phase_last(),
                    "host_numpy_s": timeit(lambda: calc_phase_host(imie, SWAVE, TH, tab, TH, WAVE), n),
                    "result_MB": got.nbytes / 1e6,
                    "max_deviation_over_column_max": float(np.max(np.abs(got - host) / np.abs(host).max(axis=1, keepdims=True)))}

    pr = syn.synth_profiles(100, S + 2, seed=11)
    zl = np.linspace(0.0, 1.0, 100)
    DUST = np.stack([2.0e3 * np.exp(-4.0 * zl), 3.0e2 * np.exp(-((zl - 0.4) / 0.1) ** 2) + 1.0e-3], axis=1)
    xs = np.linspace(0.0, 1.0, NWS)[:, None]
    KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * xs + np.arange(ND)[None])) * (1.0 + np.arange(ND)[None])
    KSCA = 0.7 * KEXT * (1.0 - 0.5 * xs)
    la = dict(NLAY=L, LAYINT=1, NINT=101)
    args = (pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)))
    dev = torch.device("cuda", eng.device)

    def pair(make_host, make_src, X):
        """median seconds of spectra_batch: the model rebuilt with the host-formed array per call against the resident source"""
        src = make_src()
        Y = src.spectra_batch(X).cpu().numpy()

        def host():
            m = make_host()
            m._sources_on = True                            # the aerosol source is resident already: only the array is formed anew
            return m.spectra_batch(X)
        same = bool(np.array_equal(host().cpu().numpy(), Y))
        t_form = timeit(lambda: make_host(), n)
        return {"host_route_s": timeit(host, n), "of_which_forming_the_array_s": t_form,
                "source_route_s": timeit(lambda: src.spectra_batch(X), n), "bit_identical": same}

    if part in ("b", "all"):
        xq, wq = np.polynomial.legendre.leggauss(5)
        MU, WT = 0.5 * (xq + 1.0), 0.5 * wq
        for tag, W, G in (("C4_W1e4_G20", 10000, 20), ("LBL_window_G1", W_lbl, 1)):
            WAVE, SWAVE = grid(W)
            PRESS, TEMP, K = torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
            if G == 1:
                eng.upload_lbltable(K.reshape(W, NP, NT, S).cpu().numpy(), PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE)
            else:
                _, delg = syn.gauss_legendre_01(G, as_float32=True)
                eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32))
            del K
            torch.cuda.empty_cache()
            st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T"])
            X = np.ascontiguousarray(perturbed_states(st.XN, 0.05 * st.XN).T[:states_b])
            dust = dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST)
            for imie in (0, 1):
                tab = np.ascontiguousarray(tables(imie, SWAVE))
                geo = (MU, WT, 2, 101, [30.0], [20.0], [45.0], np.full(W, 1.0e-8))
                kw = dict(layering_args=la, IRAY=1, IMIE=imie, dust=dust)
                mk_host = lambda: BatchedCKScatterModel(eng, st, *args, phasarr_host(imie, SWAVE, tab, WAVE), *geo, **kw)
                mk_src = lambda: BatchedCKScatterModel(eng, st, *args, None, *geo, phase_source=(imie, TH, tab), **kw)
                r = pair(mk_host, mk_src, X)
                r["states"] = int(X.shape[0]); r["phasarr_MB"] = ND * W * 2 * TH.size * 8 / 1e6
                res["scatter_batch_%s_imie%d" % (tag, imie)] = r

    if part in ("c", "all"):
        W, G = 10000, 20
        WAVE, SWAVE = grid(W)
        PRESS, TEMP, K = torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
        _, delg = syn.gauss_legendre_01(G, as_float32=True)
        eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
        st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2)])
        X = np.ascontiguousarray(perturbed_states(st.XN, 0.05 * st.XN).T)
        dust = dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST)
        solar, BRDF = 10.0 ** rng.uniform(-8, -7, W), rng.uniform(0.0, 0.15, (W, 1))
        kw = dict(layering_args=la, geometry=dict(ANGLE=20.0, EMISS_ANG=20.0), IRAY=1, dust=dust, BRDF=BRDF)
        alpha = eng.scattering_angle_deg([30.0], [20.0], [45.0])
        ray = 0.75 * (1.0 + np.cos(alpha / 180. * np.pi) ** 2) / (4.0 * np.pi)
        for imie in (0, 1, 2):
            tab = np.ascontiguousarray(tables(imie, SWAVE))

            def phase_fn_host():
                pf = np.zeros((W, 1, ND + 1))
                pf[:, :, :ND] = calc_phase_host(imie, SWAVE, TH, tab, alpha, WAVE)
                pf[:, :, ND] = ray
                return pf
            mk_host = lambda: BatchedCKSingleScatterModel(eng, st, *args, phase_fn_host(), [30.0], [20.0], solar, **kw)
            mk_src = lambda: BatchedCKSingleScatterModel(eng, st, *args, None, [30.0], [20.0], solar, phase_source=(imie, TH, tab),
                                                         AZI_ANG=[45.0], **kw)
            r = pair(mk_host, mk_src, X)
            if imie != 1:                                   # cos and pow differ by ulps between NumPy and the device
                r.pop("bit_identical")
            r["states"] = int(X.shape[0])
            res["singlescatt_batch_C2_imie%d" % imie] = r
    out["phase"] = res


def bench_scatter_cont(eng, out, W=10000, n=5):
    """C4-size scattering Jacobian (W = 1e4, G = 20, 100 layers, 8 gases, synth_cia, two aerosol populations, IRAY 4; T and one
    aerosol profile through 100 levels: 201 states) at 5 streams / NF 2 and 16 / NF 8, whole axis and the last eighth of it:
      (a) fused:   jacobian_nemesis_batched(BatchedCKScatterModel), the continuum formed inside the call;
      (b) by hand: the same Jacobian written here with what the parent of that entry has -- profiles, layer_average,
          calc_tau_cia / calc_tau_dust / calc_tau_rayleigh_batch_dev over all 20 100 layers, ContinuumRows,
          cirsrad_ck_scatter_batch_rows, the quotient.  Runs on a checkout without the fused entry too ((a) is left out).
        python tools/bench_extra.py scatter_cont [W] [repeats of (b)] [5|16: that stream count only]"""
    import torch
    import bench as B
    from archnemesis_dist_amd import layering
    from archnemesis_dist_amd.continuum_rows import ContinuumRows
    from archnemesis_dist_amd.jacobian import chunk_range, finite_difference_jacobian_dev, perturbed_states
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    nb = int(sys.argv[3]) if len(sys.argv) > 3 else n
    streams = [(5, 2), (16, 8)] if len(sys.argv) <= 4 else [s for s in [(5, 2), (16, 8)] if s[0] == int(sys.argv[4])]
    dev = torch.device("cuda", eng.device)
    G, S, L, NP, NT, NPRO, ND = 20, 8, 100, 20, 15, 100, 2
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    WAVE_all = 200.0 + (1000.0 / W) * np.arange(W)
    pr = syn.synth_profiles(NPRO, S + 2, seed=11)
    ID, ISO, igas = pr["ID"], pr["ISO"], list(range(2, S + 2))
    zl = np.linspace(0.0, 1.0, NPRO)
    DUST = np.stack([2.0e3 * np.exp(-4.0 * zl), 3.0e2 * np.exp(-((zl - 0.4) / 0.1) ** 2) + 1.0e-3], axis=1)
    SWAVE = np.linspace(0.9 * WAVE_all[0], 1.1 * WAVE_all[-1], 12)
    xs = np.linspace(0.0, 1.0, 12)[:, None]
    KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * xs + np.arange(ND)[None])) * (1.0 + np.arange(ND)[None])
    KSCA = 0.7 * KEXT * (1.0 - 0.5 * xs)
    cia = syn.synth_cia()
    TH = np.linspace(0.0, 180.0, 41); cth = np.cos(np.deg2rad(TH))
    ph = np.zeros((ND, W, 2, TH.size))
    for d, g in enumerate((0.6, 0.3)):
        ph[d, :, 0, :] = ((1 - g * g) / (1 + g * g - 2 * g * cth) ** 1.5 / (4 * np.pi))[None]
        ph[d, :, 1, :] = cth[None]
    ph = np.ascontiguousarray(ph[:, :, :, ::-1])
    la = dict(NLAY=L, LAYTYP=layering.EQUAL_LOG_PRESSURE, LAYINT=1, LAYHT=0.0, LAYANG=0.0, NINT=101)
    BASEH, BASEP = layering.layer_split(pr["RADIUS"], pr["H"], pr["P"], LAYANG=0.0, LAYHT=0.0, NLAY=L, LAYTYP=la["LAYTYP"])
    XN = np.concatenate([pr["T"], np.log(DUST[:, 0])])
    inum = np.arange(XN.size)
    sol, emi, azi = [30.0], [20.0], [45.0]
    have_fused = hasattr(eng, "cirsrad_ck_scatter_batch_cont")
    res = {"W": W, "G": G, "S": S, "L": L, "states": XN.size + 1, "median_of_fused": n, "median_of_by_hand": nb}

    def by_hand(WAVE, ws, NMU, NF, MU, WT):
        """(YN, KK) with entries of the parent commit only"""
        Wl = WAVE.size
        X = perturbed_states(XN, 0.05 * XN).T                                 # (201, NX)
        ns = X.shape[0]
        T = X[:, :NPRO].copy()
        D = np.repeat(DUST[None], ns, 0); D[:, :, 0] = np.exp(X[:, NPRO:])
        rep = lambda a: np.repeat(np.asarray(a, float)[None], ns, 0)
        o = eng.layer_average(pr["RADIUS"], rep(pr["H"]), rep(pr["P"]), T, ID, rep(pr["VMR"]), D, None, BASEH, BASEP, LAYANG=0.0,
                              LAYINT=1, LAYHT=0.0, NINT=101)
        lay = dict(zip(("HEIGHT", "PRESS", "TEMP", "TOTAM", "AMOUNT", "PP", "CONT", "FRAC", "DELH", "BASET", "LAYSF"), o))
        amount = np.ascontiguousarray(np.transpose(lay["AMOUNT"][:, :, igas], (0, 2, 1))) * 1.0e-4
        flat = lambda a: np.ascontiguousarray(a).reshape((ns * L,) + a.shape[2:])
        per_state = lambda a: np.moveaxis(a.reshape((Wl, ns, L) + a.shape[2:]), 1, 0)
        tcia = per_state(eng.calc_tau_cia(0, WAVE, cia["CIA_WAVEN"], cia["CIA_TEMP"], cia["CIA_FRAC"], cia["NPARA"], cia["K_CIA"],
                                          cia["IPAIRG1"], cia["IPAIRG2"], cia["INORMALT"], cia["INORMAL"], cia["INORMALD"], ID, ISO,
                                          flat(lay["PP"]), flat(lay["PRESS"]), flat(lay["TEMP"]), flat(lay["FRAC"]),
                                          flat(lay["TOTAM"]), flat(lay["DELH"]), with_grad=False))
        td1, tcs = eng.calc_tau_dust(WAVE, SWAVE, KEXT, KSCA, flat(lay["CONT"]))[:2]
        td1 = np.clip(np.nan_to_num(td1), 0, 1e20)
        dsum, ssum = np.sum(td1, 2), np.sum(tcs, 2)
        del td1
        frac = np.zeros_like(tcs)
        ii = np.where(ssum > 0.0)
        frac[ii[0], ii[1], :] = (tcs[ii[0], ii[1], :].T / ssum[ii[0], ii[1]]).T
        del tcs, ii
        tdust, tsca, frac = per_state(dsum), per_state(ssum), per_state(frac)
        ray = torch.empty((ns, Wl, L), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        eng.calc_tau_rayleigh_batch_dev(4, 0, np.ascontiguousarray(lay["TOTAM"]), ray, ID=ID, ISO=ISO,
                                        VMR=lay["PP"] / lay["PRESS"][:, :, None])
        eng.synchronize()
        tray = ray.cpu().numpy(); del ray
        pk = ContinuumRows(L, ND)
        for m in range(ns):
            pk.add_state(tcia[m], tdust[m], tray[m], tsca[m], np.transpose(frac[m], (0, 2, 1)))
        del tcia, tdust, tray, tsca, frac
        c1, c2 = 1.1911e-12, 1.439
        radg = np.stack([np.repeat((c1 * WAVE ** 3 / (np.exp(c2 * WAVE / lay["TEMP"][m, 0]) - 1.0))[:, None], NMU, 1) for m in range(ns)])
        Y = eng.cirsrad_ck_scatter_batch_rows(0, lay["PRESS"], lay["TEMP"], amount, pk.cont_row, pk.TAUCIA_rows, pk.TAUDUST_rows,
                                              pk.TAURAY_rows, pk.TAUSCAT_rows, ph, pk.lfrac_rows, radg, sol, emi, azi,
                                              np.full(Wl, 1.0e-8), 0, np.zeros((Wl, NMU, NMU, NF + 1)), MU, WT, NF, 101, 4, 1,
                                              wave_slice=(ws, W))
        info = (eng.last_layer_rows(), eng.last_scatter_cache(), pk.R)
        Y = torch.as_tensor(Y.reshape(ns, -1), dtype=torch.float64, device=dev)
        return finite_difference_jacobian_dev(Y, XN, inum, FIX=np.zeros(XN.size, dtype=np.int32)), info

    def times(f, reps):
        f(); ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t = time.perf_counter(); r = f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
        return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}, r

    for part, (ws, we) in (("whole_axis", (0, W)), ("one_rank_of_eight", chunk_range(W, 8, 7))):
        WAVE = WAVE_all[ws:we]
        PRESS, TEMP, K = B.torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
        K = K[ws:we].contiguous()
        eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
        torch.cuda.empty_cache()
        for NMU, NF in streams:
            xq, wq = np.polynomial.legendre.leggauss(NMU)
            MU, WT = 0.5 * (xq + 1.0), 0.5 * wq
            r = {}
            if have_fused:
                from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched
                from archnemesis_dist_amd.profile_state import ContinuousProfileState
                from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel
                st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("DUST", 0)], DUST=DUST)
                model = BatchedCKScatterModel(eng, st, pr["RADIUS"], ID, ISO, igas, ph, MU, WT, NF, 101, sol, emi, azi,
                                              np.full(we - ws, 1.0e-8), layering_args=la, IRAY=4, IMIE=1, cia=cia,
                                              dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA))
                if (ws, we) != (0, W):                            # the model on a slice: spectra_batch with the slice's place
                    whole = model.spectra_batch
                    model.spectra_batch = lambda X, device=None: whole(X, device, wave_slice=(ws, W))
                r["fused"], (YN, KK) = times(lambda: jacobian_nemesis_batched(model), n)
                r["fused_rows"], r["fused_cache"] = list(model.last_rows), list(model.last_cache)
            if nb > 0:
                r["by_hand"], ((YN_b, KK_b), info) = times(lambda: by_hand(WAVE, ws, NMU, NF, MU, WT), nb)
                r["by_hand_gas_rows"], r["by_hand_cache"], r["by_hand_continuum_rows"] = list(info[0]), list(info[1]), info[2]
                if have_fused:
                    r["fused_equals_by_hand"] = bool(np.array_equal(YN, YN_b) and np.array_equal(KK, KK_b))
            res["%s_nmu%d_nf%d" % (part, NMU, NF)] = r
    out["jacobian_C4_scatter_cont"] = res


def bench_ms_phase(eng, out, W=10000, n=2):
    """C4-size scattering Jacobian with aerosol states (W = 1e4, G = 20, 100 layers, 8 gases, two aerosol populations and
    Rayleigh): 201 profile states (the base, one layer's temperature each, one layer's gas amount each) plus 20 states that
    change population 0's phase function -- 20 variants -- and its opacity in the 10 layers that hold it; 16 streams / NF 8 and
    5 / NF 2.
      (a) variants: ONE cirsrad_ck_scatter_batch_rows call of the 221 states with phase_of / phasarr_variants;
      (b) parent:   what a checkout without the keywords does for the same states -- one batched call of the 201 states that
          share the phase function plus one batched call of one model per aerosol state.  Runs on such a checkout too ((a) is
          left out there).
        python tools/bench_extra.py ms_phase [W] [repeats] [5|16: that stream count only]"""
    import torch
    import bench as B
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    n = int(sys.argv[3]) if len(sys.argv) > 3 else n
    streams = [(16, 8), (5, 2)] if len(sys.argv) <= 4 else [s for s in [(16, 8), (5, 2)] if s[0] == int(sys.argv[4])]
    dev = torch.device("cuda", eng.device)
    G, S, L, NP, NT, ND, NV, LAYERS = 20, 8, 100, 20, 15, 2, 20, range(40, 50)
    rng = np.random.default_rng(20261021)
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    WAVE = 200.0 + (1000.0 / W) * np.arange(W)
    PRESS, TEMP, K = B.torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
    eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
    torch.cuda.empty_cache()
    atm = syn.synth_atmosphere(L, S, seed=2)
    lay_p, lay_t, amount = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    # the continuum by rows: the base's 100 layers, then 10 rows per aerosol state
    R = L + NV * len(LAYERS)
    sc = np.zeros((R, ND, W))                                               # scattering opacity by population
    sc[:L, 1] = 10.0 ** rng.uniform(-4, -2, (L, W))
    for l in LAYERS:
        sc[l, 0] = 10.0 ** rng.uniform(-3, -1.5, W)
    cia = np.zeros((R, W)); ray = np.zeros((R, W))
    cia[:L] = 10.0 ** rng.uniform(-5, -2, (L, W)); ray[:L] = 10.0 ** rng.uniform(-6, -3, (L, W))
    n_prof, ns = 2 * L + 1, 2 * L + 1 + NV
    cont_row = np.tile(np.arange(L, dtype=np.int32), (ns, 1))
    for j in range(NV):
        rows = L + j * len(LAYERS) + np.arange(len(LAYERS))
        sc[rows] = sc[list(LAYERS)]; sc[rows, 0] *= 1.0 + 0.02 * (j + 1)
        cia[rows] = cia[list(LAYERS)]; ray[rows] = ray[list(LAYERS)]
        cont_row[n_prof + j, list(LAYERS)] = rows
    sca = sc.sum(axis=1)
    dust = sca * 1.2
    frac = np.where(sca[:, None, :] > 0, sc / np.where(sca > 0, sca, 1.0)[:, None, :], 0.0)
    del sc
    lp = np.tile(lay_p, (ns, 1)); lt = np.tile(lay_t, (ns, 1)); am = np.tile(amount, (ns, 1, 1))
    for k in range(L):
        lt[1 + k, k] *= 1.01
        am[1 + L + k, k % S, k] *= 1.05
    TH = np.linspace(0.0, 180.0, 41); cth = np.cos(np.deg2rad(TH))
    hg = lambda g: (1 - g * g) / (1 + g * g - 2 * g * cth) ** 1.5 / (4 * np.pi)

    def phasarr(g0):
        ph = np.zeros((ND, W, 2, TH.size))
        ph[0, :, 0, :] = hg(g0)[None]; ph[1, :, 0, :] = hg(0.3)[None]; ph[:, :, 1, :] = cth[None, None]
        return np.ascontiguousarray(ph[:, :, :, ::-1])
    ph = [phasarr(0.6)] + [phasarr(0.6 + 0.01 * (j + 1)) for j in range(NV)]
    phase_of = np.concatenate([np.zeros(n_prof, dtype=np.int32), 1 + np.arange(NV, dtype=np.int32)])
    have = bool(getattr(eng, "scatter_phase_variants", False))
    res = {"W": W, "G": G, "S": S, "L": L, "states": ns, "variants": NV, "layers_with_the_changed_population": len(LAYERS),
           "median_of": n}

    def times(f):
        f(); ts = []
        for _ in range(n):
            torch.cuda.synchronize(); t = time.perf_counter(); r = f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
        return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}, r

    for NMU, NF in streams:
        xq, wq = np.polynomial.legendre.leggauss(NMU)
        MU, WT = 0.5 * (xq + 1.0), 0.5 * wq
        c1, c2 = 1.1911e-12, 1.439
        radg = np.repeat((c1 * WAVE ** 3 / (np.exp(c2 * WAVE / lay_t[0]) - 1.0))[:, None], NMU, 1)
        tail = ([30.0], [20.0], [45.0], np.full(W, 1.0e-8), 0, np.zeros((W, NMU, NMU, NF + 1)), MU, WT, NF, 101, 1, 1)

        def call(sel, phasarr0, **kw):
            return eng.cirsrad_ck_scatter_batch_rows(0, lp[sel], lt[sel], am[sel], cont_row[sel], cia, dust, ray, sca, phasarr0, frac,
                                                     np.tile(radg, (len(lp[sel]), 1, 1)), *tail, **kw)

        def parent():
            parts = [call(slice(0, n_prof), ph[0])]
            walk = [eng.last_scatter_walk_ms()] if have else []
            for j in range(NV):
                parts.append(call(slice(n_prof + j, n_prof + j + 1), ph[1 + j]))
            return np.concatenate(parts), walk

        r = {}
        r["parent_route"], (Yp, walk_p) = times(parent)
        if walk_p:
            r["parent_route_walk_ms_of_the_201_state_call"] = walk_p[0]
        if have:
            def variants():
                Y = call(slice(None), ph[0], phase_of=phase_of, phasarr_variants=np.stack(ph[1:]))
                return Y, eng.last_scatter_cache(), eng.last_scatter_variants(), eng.last_scatter_walk_ms()
            r["variants"], (Yv, cache, (pairs, nbytes), walk_ms) = times(variants)
            r["variants_cache"], r["variants_pairs"], r["variants_buffer_bytes"], r["variants_walk_ms"] = list(cache), pairs, nbytes, walk_ms
            r["variants_equal_parent_route"] = bool(np.array_equal(Yv, Yp))
        res["nmu%d_nf%d" % (NMU, NF)] = r
    out["jacobian_C4_ms_phase"] = res


def bench_next(eng, out, rng):
    """the "next" rows: ILS convolution of an LBL spectrum with gradients, continuum opacities at C2, the
    k-table generator's binning -- host arrays in / out, beside the NumPy oracle where it finishes in seconds"""
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    # ILS: 1e6-point spectrum + 100 gradient columns, 1000 convolution points, Gaussian FWHM 0.4 cm-1 (~800 points a window)
    nw, nx, nc = 1000000, 100, 1000
    vw = 2000.0 + 1e-3 * np.arange(nw)
    y = rng.uniform(1, 2, nw); dy = rng.normal(size=(nw, nx))
    vc = np.linspace(2001.0, 2999.0, nc)
    t = timeit(lambda: eng.lblconvg(nw, vw, y, dy, nc, vc, 2, 0.4), 2)
    sub = slice(0, 20)
    t0 = time.perf_counter(); orc.lblconv(nw, vw, y, 20, vc[sub], 2, 0.4, dydx=dy); to = (time.perf_counter() - t0) * nc / 20
    out["lblconvg_1e6x100grad_1000conv"] = {"gpu_wall_s_host_arrays": t, "numpy_oracle_s_extrapolated_from_20_points": to}
    # continuum at C2: CIA table 2 pairs, Rayleigh (Jovian air), 2 aerosol populations
    W, L = 10000, 100
    wn = 200.0 + 0.1 * np.arange(W)
    TOTAM = 10.0 ** rng.uniform(24, 28, L)
    ID = np.array([39, 40, 6, 11]); ISO = np.zeros(4, int); VMR = np.tile([0.86, 0.13, 2e-3, 1e-4], (L, 1))
    tr = timeit(lambda: eng.calc_tau_rayleigh(4, 0, wn, TOTAM, ID, ISO, VMR))
    SW = np.linspace(150.0, 1300.0, 40); KE = 10.0 ** rng.uniform(-10, -8, (40, 2)); KS = KE * 0.6
    CONT = 10.0 ** rng.uniform(3, 8, (L, 2))
    td = timeit(lambda: eng.calc_tau_dust(wn, SW, KE, KS, CONT))
    t0 = time.perf_counter(); orc.calc_tau_dust(wn, SW, KE, KS, CONT); tdo = time.perf_counter() - t0
    out["continuum_C2"] = {"rayleigh_ls_gpu_s": tr, "dust_2pop_gpu_s": td, "dust_scipy_oracle_s": tdo}
    # k-table generator: 200 bins of ~2.5e4 line-by-line points (overlapping ILS windows), 20 g-ordinates
    n = 2000000
    w = np.linspace(1000.0, 1100.0, n)
    k = 10.0 ** (-24 + 3 * np.sin(w * 11.0) ** 2 + rng.normal(0, 0.3, n))
    cen = np.linspace(1001.0, 1099.0, 200); half = np.full(200, 0.625)
    x, _ = np.polynomial.legendre.leggauss(20); g = 0.5 * (x + 1)
    tk = timeit(lambda: eng.kdist_bins(w, k, cen - half, cen + half, g), 2)
    t0 = time.perf_counter(); orc.kdist_bins(w, k, cen - half, cen + half, g); tko = time.perf_counter() - t0
    out["kdist_200bins_2.5e4pts"] = {"gpu_wall_s_host_arrays": tk, "numpy_oracle_s": tko}


def bench_ss(eng, out, rng, runs=5):
    """Numerical Jacobian of a single-scattering configuration (ISCAT = 3) at C2 size: 201 forward models (T and ln VMR of one
    absorber at 100 levels through Curtis-Godson layer_average, as the c4 / grad workloads build them), the synthetic scattering
    inputs of tests/test_gpu_parity.py::_singlescatt_vs_oracle at 1e4 wavenumbers x 100 layers.  (a) one
    cirsrad_ck_singlescatt call per state against (b) ONE cirsrad_ck_singlescatt_batch call; host arrays in / out, medians of
    `runs` rounds after a warm-up, the order of (a) and (b) swapped from round to round."""
    import torch
    from archnemesis_dist_amd.jacobian import perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    from bench import torch_ktable
    W, G, S, L, NP, NT = 10000, 20, 8, 100, 20, 15
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    PRESS, TEMP, K = torch_ktable(torch, torch.device("cuda", 0), W, G, NP, NT, S, seed=20260704)
    WAVE = 200.0 + 0.1 * np.arange(W)
    eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
    pr = syn.synth_profiles(100, S + 2, seed=11)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2)])
    model = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)),
                                  layering_args=dict(NLAY=L, LAYINT=1, NINT=101))
    X = perturbed_states(st.XN, 0.05 * st.XN).T
    lay = model.layers(X)
    lp, lt, am = (np.ascontiguousarray(lay[k]) for k in ("PRESS", "TEMP", "amount"))
    n = X.shape[0]
    TAURAY = 10.0 ** rng.uniform(-4, -2, (W, L)); TAUSCAT = 10.0 ** rng.uniform(-3, -1, (W, L)); TAUSCAT[:, 4] = 0.0
    cont = 10.0 ** rng.uniform(-5, -3, (W, L)) + 1.2 * TAUSCAT + TAURAY
    sca = TAURAY + TAUSCAT
    phase = 10.0 ** rng.uniform(-1.5, 0.3, (1, W, L))
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 20.0)
    EMTEMP = lt[:, LAYINC[:, 0]][:, :, None]
    EMIS = rng.uniform(0.7, 1.0, W); BRDF = rng.uniform(0.0, 0.15, (W, 1)); SOLF = 10.0 ** rng.uniform(-8, -7, W)
    tail = (EMIS, BRDF, SOLF, [30.0], [20.0])
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[None], (n,) + a.shape))

    def separate():
        return np.stack([eng.cirsrad_ck_singlescatt(0, lp[m], lt[m], am[m], cont, sca, phase, NLAYIN, LAYINC, SCALE, EMTEMP[m], -1.0, *tail)
                         for m in range(n)])
    res = {"what": "numerical Jacobian, single scattering (ISCAT = 3) at C2 size: %d forward models, W=1e4, L=100, S=8, G=20, one "
                   "path; host arrays in / out" % n, "forward_models": n, "runs": runs}
    batched = None
    if hasattr(eng, "cirsrad_ck_singlescatt_batch"):
        contn, scan, phasen, scalen = rep(cont), rep(sca), rep(phase), rep(SCALE)
        tsurf = np.full(n, -1.0)
        batched = lambda: eng.cirsrad_ck_singlescatt_batch(0, lp, lt, am, contn, scan, phasen, NLAYIN, LAYINC, scalen, EMTEMP, tsurf, *tail)
    ref = separate()                                            # warm-up of both
    ta, tb, parts = [], [], []
    if batched:
        res["bit_identical_to_separate_calls"] = bool(np.array_equal(batched(), ref))
    for r in range(runs):
        for which in (("a", "b") if r % 2 == 0 else ("b", "a")):
            if which == "b" and not batched:
                continue
            t = time.perf_counter(); (separate if which == "a" else batched)(); dt = time.perf_counter() - t
            (ta if which == "a" else tb).append(dt)
            if which == "b":
                parts.append(eng.last_kernel_ms())
    res["separate_calls_wall_s"] = float(np.median(ta)); res["separate_calls_wall_s_all"] = ta
    if batched:
        res["batch_wall_s"] = float(np.median(tb)); res["batch_wall_s_all"] = tb
        res["speedup"] = res["separate_calls_wall_s"] / res["batch_wall_s"]
        res["batch_gas_opacity_kernel_ms"] = float(np.median([k["overlap_ms"] for k in parts]))
        res["batch_rt_kernel_ms"] = float(np.median([k["rt_ms"] for k in parts]))      # flags, state 0's pass, the other states
        res["gas_opacity_rows"] = list(eng.last_layer_rows()); res["rt_shared"] = bool(eng.last_rt_shared())
        nbytes = contn.nbytes + scan.nbytes + phasen.nbytes
        th = []
        for _ in range(3):                                      # what the upload of one per-model array costs, pageable host memory
            torch.cuda.synchronize(); t = time.perf_counter(); d = torch.from_numpy(contn).to("cuda:0"); torch.cuda.synchronize()
            th.append(time.perf_counter() - t); del d
        res["per_model_arrays_GB"] = nbytes / 1e9
        res["h2d_pageable_GB_per_s"] = contn.nbytes / 1e9 / float(np.median(th))
        res["upload_estimate_s"] = nbytes / 1e9 / res["h2d_pageable_GB_per_s"]
    out["singlescatt_jacobian_C2"] = res


def bench_ss_cont(eng, out, rng, runs=5):
    """The 201 states of the `ss` workload with real sources: synth_cia, two aerosol populations, IRAY 1, one path.  From the
    layers of the states on the host,
      (a) array level: calc_tau_cia / calc_tau_dust / calc_tau_rayleigh over all 20 100 layers, the sums and the phase mix in NumPy
          (scatter_state.singlescatt_dense_by_hand), then cirsrad_ck_singlescatt_batch on the dense arrays;
      (b) fused: cirsrad_ck_singlescatt_batch_cont, the three arrays formed per distinct layer inside the call.
    Medians of `runs` rounds after a warm-up of both, the order of (a) and (b) swapped from round to round.
        python tools/bench_extra.py ss_cont [runs]"""
    import torch
    from archnemesis_dist_amd.jacobian import perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKSingleScatterModel, singlescatt_dense_by_hand
    from bench import torch_ktable
    if len(sys.argv) > 2:
        runs = int(sys.argv[2])
    W, G, S, L, NP, NT, ND = 10000, 20, 8, 100, 20, 15, 2
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    PRESS, TEMP, K = torch_ktable(torch, torch.device("cuda", 0), W, G, NP, NT, S, seed=20260704)
    WAVE = 200.0 + 0.1 * np.arange(W)
    eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
    pr = syn.synth_profiles(100, S + 2, seed=11)
    zl = np.linspace(0.0, 1.0, 100)
    DUST = np.stack([2.0e3 * np.exp(-4.0 * zl), 3.0e2 * np.exp(-((zl - 0.4) / 0.1) ** 2) + 1.0e-3], axis=1)
    SWAVE = np.linspace(0.9 * WAVE[0], 1.1 * WAVE[-1], 12)
    xs = np.linspace(0.0, 1.0, 12)[:, None]
    KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * xs + np.arange(ND)[None])) * (1.0 + np.arange(ND)[None])
    KSCA = 0.7 * KEXT * (1.0 - 0.5 * xs)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2)])
    phase_fn = 10.0 ** rng.uniform(-1.5, 0.3, (W, 1, ND + 1))
    model = BatchedCKSingleScatterModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)), phase_fn, [30.0], [20.0],
                                        10.0 ** rng.uniform(-8, -7, W), layering_args=dict(NLAY=L, LAYINT=1, NINT=101),
                                        geometry=dict(ANGLE=20.0, EMISS_ANG=20.0), IRAY=1, cia=syn.synth_cia(),
                                        dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST), BRDF=rng.uniform(0.0, 0.15, (W, 1)),
                                        emissivity=rng.uniform(0.7, 1.0, W))
    model.upload_sources()
    X = perturbed_states(st.XN, 0.05 * st.XN).T
    lay = model.layers(X)
    n = X.shape[0]
    path = lay["path"]
    rt = (path.NLAYIN, path.LAYINC, np.repeat(path.SCALE[None], n, 0), path.EMTEMP, np.full(n, -1.0), model.emissivity, model.BRDF,
          model.solar, model.SOL_ANG, model.EMISS_ANG)
    small = [lay[k] for k in ("PRESS", "TEMP", "amount", "VMRLAY", "FRAC", "TOTAM", "DELH", "CONT")] + [rt[2], rt[3]]
    info = {}

    def array_level():
        t = time.perf_counter()
        d = singlescatt_dense_by_hand(eng, 0, 1, model.ID, model.ISO, model.cia, model.dust, lay, phase_fn)
        info["a_formation_s"] = time.perf_counter() - t
        info["a_bytes"] = sum(a.nbytes for a in d) + sum(a.nbytes for a in small[:3] + small[8:])
        return eng.cirsrad_ck_singlescatt_batch(0, lay["PRESS"], lay["TEMP"], lay["amount"], *d, *rt)

    def fused():
        return eng.cirsrad_ck_singlescatt_batch_cont(0, lay["PRESS"], lay["TEMP"], lay["amount"], lay["VMRLAY"], lay["FRAC"], lay["TOTAM"],
                                                     lay["DELH"], lay["CONT"], 1, None, phase_fn, *rt)
    res = {"what": "numerical Jacobian, single scattering (ISCAT = 3) at C2 size with CIA, two aerosol populations and IRAY 1: %d "
                   "forward models, W=1e4, L=100, S=8, G=20, one path; host arrays in / out" % n, "forward_models": n, "runs": runs}
    ref = array_level()
    res["bit_identical"] = bool(np.array_equal(fused(), ref))
    ta, tb, fa, ka, kb = [], [], [], [], []
    for r in range(runs):
        for which in (("a", "b") if r % 2 == 0 else ("b", "a")):
            t = time.perf_counter(); (array_level if which == "a" else fused)(); dt = time.perf_counter() - t
            (ta if which == "a" else tb).append(dt)
            (ka if which == "a" else kb).append(eng.last_kernel_ms())
            if which == "a":
                fa.append(info["a_formation_s"])
            else:
                res["fused_rows"] = list(eng.last_layer_rows()); res["fused_rt_shared"] = bool(eng.last_rt_shared())
    med = lambda v: float(np.median(v))
    res["array_level_wall_s"] = med(ta); res["array_level_wall_s_all"] = ta
    res["array_level_formation_s"] = med(fa); res["array_level_dense_entry_s"] = med([a - f for a, f in zip(ta, fa)])
    res["fused_wall_s"] = med(tb); res["fused_wall_s_all"] = tb
    res["speedup"] = res["array_level_wall_s"] / res["fused_wall_s"]
    for tag, ks in (("array_level", ka), ("fused", kb)):
        res[tag + "_gas_opacity_kernel_ms"] = med([k["overlap_ms"] for k in ks])
        res[tag + "_rt_kernel_ms"] = med([k["rt_ms"] for k in ks])
    res["array_level_input_GB"] = info["a_bytes"] / 1e9
    res["fused_input_GB"] = (sum(a.nbytes for a in small) + phase_fn.nbytes) / 1e9
    out["singlescatt_jacobian_C2_cont"] = res


def bench_maps(eng, out, rng):
    # ---- nemesisfmg tail at C2: map2pro + map2xvec, host arrays in / out vs NumPy on the host ---------------
    W, NVMR, NDUST, Li, NPRO, NX = 10000, 8, 0, 100, 100, 200
    NPAR = NVMR + 2 + NDUST
    dS = rng.normal(size=(W, NPAR, Li, 1))
    LAYINC = np.arange(Li, dtype=np.int32)[::-1].copy()[:, None]
    DTE, DAM, DCO = (rng.uniform(0, 1, (Li, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    NLAYIN = np.array([Li], dtype=np.int32)

    def gpu():
        p = eng.map2pro(dS, W, NVMR, NDUST, NPRO, 1, NLAYIN, LAYINC, DTE, DAM, DCO)
        return eng.map2xvec(p, W, NVMR, NDUST, NPRO, 1, NX, xmap)

    def host():
        p = np.zeros((W, NPAR, NPRO, 1))
        last = None
        for par in range(NPAR):
            M = DAM if par < NVMR else (DTE if par == NVMR else (DCO if par <= NVMR + NDUST else None))
            if M is not None:
                last = np.tensordot(dS[:, par, :, 0], M[LAYINC[:, 0], :], axes=(1, 0))
            p[:, par, :, 0] = last          # para-H2 slot: the reference's stale dSPECOUT1
        return np.tensordot(p, xmap, axes=([1, 2], [1, 2]))
    tg = timeit(gpu)
    th = timeit(host, n=2)
    err = float(np.max(np.abs(gpu() - host())) / np.max(np.abs(host())))
    out["gradient_maps_C2"] = {"gpu_wall_s_host_ptr": tg, "numpy_host_wall_s": th, "max_rel_diff": err,
                               "note": "W=1e4, NPAR=10, Li=100, NPRO=100, NX=200; GPU time includes 80 MB H2D + 96 MB D2H"}


def bench_grad(eng, out):
    # ---- analytic Jacobian at C2 ------------------------------------------------------------------
    W, G, S, L, NP, NT = 10000, 20, 8, 100, 20, 15
    _, delg = syn.gauss_legendre_01(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S)
    WAVE = 200.0 + 0.1 * np.arange(W)
    eng.upload_ktable(K, PRESS, TEMP, WAVE, delg); del K
    atm = syn.synth_atmosphere(L, S)
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L)
    EMTEMP = atm["lay_temp"][:, LAYINC[:, 0]][:, :, None]
    NVMR, NPAR = S, S + 2
    ig = np.arange(S, dtype=np.int32)
    f = lambda: eng.cirsradg_ck_thermal(0, atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0], None, None, NVMR, NPAR,
                                        ig, NLAYIN, LAYINC, SCALE, EMTEMP[0], -1.0)
    t = timeit(f)
    k = eng.last_kernel_ms()
    out["cirsradg_C2"] = {"wall_s_host_ptr": t, "overlapg_kernel_ms": k["overlap_ms"], "rtg_kernel_ms": k["rt_ms"],
                          "note": "W=1e4,L=100,S=8,G=20, NPAR=10: SPECOUT + dSPECOUT(1e4,10,100,1) + dTSURF"}


def bench_ms(eng, out, rng):
    # ---- multiple scattering, C4-like -----------------------------------------------------------------
    Wm, Gm, Lm, M, NF, NC = 256, 20, 100, 16, 8, 1
    x, w = np.polynomial.legendre.leggauss(2 * M)
    mu1 = np.sort(np.abs(x[x > 0])); wt1 = w[x > 0][np.argsort(np.abs(x[x > 0]))]
    TH = np.linspace(0, 180, 41)
    ph = np.zeros((NC, Wm, 2, TH.size)); c = np.cos(np.deg2rad(TH))
    ph[:, :, 0, :] = ((1 - 0.36) / (1 + 0.36 - 1.2 * c) ** 1.5 / (4 * np.pi))[None, None, :]
    ph[:, :, 1, :] = c[None, None, :]
    ph = np.ascontiguousarray(ph[:, :, :, ::-1])
    taus = 10.0 ** rng.uniform(-3, 0.5, (Wm, Gm, Lm)); tauray = 10.0 ** rng.uniform(-6, -3, (Wm, Lm))
    tausc = 10.0 ** rng.uniform(-4, -1, (Wm, Lm)); taus = np.maximum(taus, (tausc + tauray)[:, None, :] * 1.05)
    om = np.broadcast_to((tausc + tauray)[:, None, :], taus.shape) / taus
    args = (ph, np.full((Wm, M), 1e-7), np.array([30.0]), np.array([20.0]), np.full(Wm, 1e-8), np.array([45.0]), 0,
            np.zeros((Wm, M, M, NF + 1)), mu1, wt1, NF, 500.0 + np.arange(Wm), np.full((Wm, Lm), 1e-7), taus, tauray, om, 101, 1, 1,
            np.ones((Wm, NC, Lm)))
    t = timeit(lambda: eng.scloud11wave_core(*args), n=2)
    nn = np.maximum((np.log2(taus) + 12).astype(int), 0)
    flops = float(((nn * 6.67 + 5) * 2 * M ** 3).sum() * (NF + 1))
    out["scloud11wave_C4like"] = {"wall_s": t, "waves": Wm, "g": Gm, "layers": Lm, "nmu": M, "nf": NF,
                                  "approx_flops": flops, "TFLOPs": flops / t / 1e12,
                                  "scaled_to_W1e4_s": t * 1e4 / Wm}


def bench_lbl(eng, out, rng, full=False):
    # ---- runtime LBL: reduced C5 (default) or the full C5 grid (1e6 wavenumbers x 50 layers, 1e5 lines) ---------
    nw, N, Ll = (1000000, 100000, 50) if full else (200000, 20000, 5)
    wn = 2000.0 + 1e-3 * np.arange(nw)
    span = nw * 1e-3
    nu = np.sort(rng.uniform(2000.0 - 75.0, 2000.0 + span + 75.0, N)); sw = 10.0 ** rng.uniform(-28, -19, N); el = rng.uniform(0, 3000, N)
    bp = np.zeros((3, N)); bp[0] = rng.uniform(0.02, 0.1, N); bp[1] = rng.uniform(0.5, 0.8, N); bp[2] = rng.uniform(-0.01, 0.01, N)
    c2 = 2.99792458E10 * 6.62607015E-27 / 1.380649E-16
    sr = 1 - np.exp(-c2 * nu / 296.0)
    tt = np.linspace(150, 300, Ll); pp = np.logspace(-4, 0, Ll); qq = np.ones(Ll)
    o = np.zeros((Ll, nw))
    t = timeit(lambda: eng.add_line_set_monochromatic_absorption(wn, 0, tt, 296.0, pp, 1.0, qq, 1.0, 28.0, np.array([1.0]), bp, nu,
                                                                 sw, el, sr, o), n=2)
    evals = float(N) * (150.0 / 1e-3) * Ll * (span / (span + 150.0))     # lines whose window overlaps the grid, roughly
    out["lbl_runtime_C5" if full else "lbl_runtime_reducedC5"] = {"wall_s": t, "grid": nw, "lines": N, "layers": Ll, "approx_profile_evals": evals,
                                    "Gevals_per_s": evals / t / 1e9}


def bench_lbl_pc(eng, out, nw=1000000, Ll=50, lines=100000, n_iso=3, n=5):
    """the pseudo-continuum of the weak lines at C5 size (1e6 points x 50 layers, 1 cm-1 bins over the grid +- 150 cm-1) beside
    the line call of the same process, and a gas of three isotopologues (lines + pseudo-continuum each) through the
    accumulator against the same six host-array calls; medians of n after one warm-up"""
    if len(sys.argv) > 2:                                    # reduced sizes for a quick look: lbl_pc <points> <layers>
        nw, Ll = int(sys.argv[2]), int(sys.argv[3])
        lines = max(nw // 10, 100)
    wn = 2000.0 + 1e-3 * np.arange(nw)
    tt = np.linspace(150, 300, Ll); pp = np.logspace(-4, 0, Ll)
    gas = syn.synth_lbl_gas(wn[0], wn[-1], n_iso, lines, Ll, seed=0)
    o = np.zeros((Ll, nw))
    ln, ct = gas[0]
    t_pc = timeit(lambda: eng.add_pseudo_continuum_monochromatic_absorption(wn, ct[0], tt, ct[1], pp, *ct[2:], o), n)
    t_ln = timeit(lambda: eng.add_line_set_monochromatic_absorption(wn, ln[0], tt, ln[1], pp, *ln[2:], o), n)

    def host_chain():
        o[...] = 0.0
        for a, b in gas:
            eng.add_line_set_monochromatic_absorption(wn, a[0], tt, a[1], pp, *a[2:], o)
            eng.add_pseudo_continuum_monochromatic_absorption(wn, b[0], tt, b[1], pp, *b[2:], o)
        return o

    def accumulated(read=True):
        acc = eng.lbl_accumulator(wn, tt, pp)
        for a, b in gas:
            acc.add_lines(*a)
            acc.add_pseudo_continuum(*b)
        if read:
            return acc.numpy()
        eng.synchronize()

    t_host = timeit(host_chain, n)
    t_acc = timeit(accumulated, n)
    t_dev = timeit(lambda: accumulated(False), n)
    same = bool(np.array_equal(accumulated(), host_chain()))
    out["lbl_pc_C5" if (nw, Ll) == (1000000, 50) else "lbl_pc_reduced"] = {
        "grid": nw, "layers": Ll, "bins": int(ct[8].size), "lines": lines, "isotopologues": n_iso, "median_of": n,
        "pseudo_continuum_call_wall_s": t_pc, "line_call_wall_s": t_ln,
        "gas_host_array_calls_wall_s": t_host, "gas_accumulator_wall_s": t_acc, "gas_accumulator_left_in_hbm_wall_s": t_dev,
        "accumulator_equals_host_calls": same}


def bench_lblrt(eng, out, nw=1000000, Ll=50, lines=100000, n_iso=3, n=3):
    """CIRSrad's thermal branch on runtime line-by-line opacities at C5 size (1e6 points x 50 layers, one gas of three
    isotopologues with 1e5 lines each), end to end: the line source resident in HBM (pack the rows, set the state, the call)
    beside what the same opacities cost through the per-call entries -- 2 n_iso accumulator adds that stage the line list
    each time, the read-back, an LBL-table-style upload of the result and the same call on it.  Medians of n after one
    warm-up; `lblrt <points> <layers>` for a quick look."""
    from archnemesis_dist_amd import line_source as ls
    if len(sys.argv) > 3:
        nw, Ll = int(sys.argv[2]), int(sys.argv[3])
        lines = max(nw // 10, 100)
    wn = 2000.0 + 1e-3 * np.arange(nw)
    src = syn.synth_line_source(wn, (n_iso,), lines, seed=0)
    lp = 101325.0 * np.logspace(-4, 0, Ll)[::-1].copy(); lt = np.linspace(300.0, 150.0, Ll)
    am = np.full((1, Ll), 1.0e22) * (lp / lp[0])[None, :]
    mix = np.array([[0.05, 0.95]])
    NLAYIN, LAYINC, SCALE = syn.nadir_path(Ll, 10.0)
    EMTEMP = lt[LAYINC[:, 0]][:, None]
    cont = np.zeros((nw, Ll))
    thermal = lambda: eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, -1.0)
    t_up = timeit(lambda: eng.upload_line_source(src), 1)

    def resident(grad=False):
        eng.set_line_state(ls.pack_line_state(src, lp / 101325.0, lt, mix, grad=grad))
        return thermal()

    def state_only():
        eng.set_line_state(ls.pack_line_state(src, lp / 101325.0, lt, mix))
        eng.synchronize()

    t_res = timeit(resident, n)
    t_state = timeit(state_only, n)
    spec = resident()
    t_res_g = timeit(lambda: resident(True), 1)
    ql, qc = ls.q_ratios(src, np.zeros(Ll, dtype=int), lt)
    ql, qc = ql.reshape(Ll, -1), qc.reshape(Ll, -1)

    def per_call_entries():
        acc = eng.lbl_accumulator(wn, lt, lp / 101325.0)
        for i, iso in enumerate(src.gases[0]):
            acc.add_lines(0, iso.t_ref, iso.p_ref, ql[:, i], iso.abundance, iso.mass, mix[0], iso.bparams, iso.nu, iso.sw, iso.e_lower,
                          iso.stim_ref)
            acc.add_pseudo_continuum(0, iso.t_cont, iso.p_cont, qc[:, i], iso.abundance, iso.mass, mix[0], iso.pc_bparams, iso.centers,
                                     iso.widths, iso.sw_sum, iso.pc_e_lower)
        k = acc.numpy()                                                             # (L, nw)
        K = np.ascontiguousarray(np.repeat(k.T[:, :, None, None], 2, axis=2))       # (W, NP = L, NT = 2, S = 1)
        eng.upload_lbltable(K, (lp / 101325.0)[::-1].copy(), np.array([100.0, 400.0]), wn)
        return thermal()

    t_old = timeit(per_call_entries, n)
    eng.upload_line_source(src)
    out["lblrt_C5" if (nw, Ll) == (1000000, 50) else "lblrt_reduced"] = {
        "grid": nw, "layers": Ll, "lines": lines, "isotopologues": n_iso, "median_of": n,
        "line_source_upload_wall_s": t_up, "cirsrad_thermal_on_line_source_wall_s": t_res,
        "of_which_pack_and_set_state_wall_s": t_state, "with_T_plus_5_rows_wall_s": t_res_g,
        "per_call_entries_readback_table_upload_wall_s": t_old, "ratio": t_old / t_res,
        "spectrum_finite": bool(np.all(np.isfinite(spec)))}


def bench_mie(eng, out, nwave=64, n=5):
    """Scatter_0.makephase for one size distribution: 64 wavelengths over 0.4 - 5 um, log-normal (1.0, 0.4), m = 1.4 - 0.01i, the
    reference's default 41 angles folded to <= 90 degrees (21), open range at the default step 0.015 lambda_min.  Kernel time
    (hipEvents around each block's launches), the call end to end, the radii per wavelength, and the NumPy restatement of
    tests/mie_cases.py on 4 of the wavelengths -- NOT a comparator: the reference runs numba-compiled loops, the
    restatement is pure NumPy."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mie_cases as mc
    wavel = np.exp(np.linspace(np.log(0.4), np.log(5.0), nwave))
    theta = np.array([0, 1, 2, 3, 4, 5, 7.5, 10, 12.5, 15, 17.5, 20, 25, 30, 35, 40, 50, 60, 70, 80, 90.0])
    dsize, rs = np.array([1.0, 0.4, 0.0]), np.array([0.015 * wavel.min(), 0.0, 0.015 * wavel.min()])
    refindx = np.tile([1.4, 0.01], (nwave, 1))
    res = {}
    for block in (None, 64, 2048):
        run = lambda: eng.mie_makephase(wavel, 2, dsize, rs, refindx, theta, radius_block=block, return_counts=True)
        wall = timeit(run, n)
        ms, blocks, radii = eng.mie_last()
        res["block %s" % (block or "default")] = {"end_to_end_ms": 1e3 * wall, "kernel_ms": ms, "blocks": blocks, "block_radii": radii}
    xs, xe, thetax, ph, counts = eng.mie_makephase(wavel, 2, dsize, rs, refindx, theta, return_counts=True)
    pick = [0, nwave // 3, 2 * nwave // 3, nwave - 1]
    t = time.perf_counter()
    hs, he, _, hp, hc = mc.makephase_np(wavel[pick], 2, dsize, rs, refindx[pick], theta, chunk_order=True, return_counts=True)
    host = time.perf_counter() - t
    res["radii_min_max"] = [int(counts.min()), int(counts.max())]
    res["radii_total"] = int(counts.sum())
    res["host_restatement_s_per_wavelength_not_representative"] = host / len(pick)
    res["host_vs_gpu"] = {"counts_equal": bool(np.array_equal(hc, counts[pick])),
                          "xext_rel": float(np.max(np.abs(xe[pick] / he - 1))), "phas_rel": float(np.max(np.abs(ph[pick] / hp - 1)))}
    out["mie_lognormal_64_wavelengths"] = res
    # ... and what follows it with IMIE = 0: the double Henyey-Greenstein fit of the 64 phase functions at the 41 angles
    # (Scatter_0.subfithgm).  Kernel time from hg_fit_last, the median of n calls end to end, the calls of mrqminl per fit,
    # and the NumPy restatement of tests/hgfit_cases.py on the same 64 fits -- NOT a comparator either.
    import hgfit_cases as hg
    run = lambda: eng.hg_fit(thetax, ph, return_counts=True)
    wall = timeit(run, n)
    kernel_ms = eng.hg_fit_last()
    f, g1, g2, rms, calls = run()
    t = time.perf_counter()
    host_fit = hg.subfithgm_np(thetax, ph, order="kernel", return_counts=True)
    host = time.perf_counter() - t
    dev = hg.deviations((f, g1, g2, rms), host_fit)
    out["hg_fit_64_wavelengths_41_angles"] = {
        "end_to_end_ms": 1e3 * wall, "kernel_ms": kernel_ms, "median_of": n, "angles": int(thetax.shape[0]),
        "calls_min_median_max": [int(calls[:, 0].min()), int(np.median(calls[:, 0])), int(calls[:, 0].max())],
        "accepted_min_max": [int(calls[:, 1].min()), int(calls[:, 1].max())], "calls_total": int(calls[:, 0].sum()),
        "host_restatement_s_all_fits_not_a_comparator": host,
        "host_vs_gpu": {"calls_equal": bool(np.array_equal(host_fit[4], calls)), "params_rel": dev[0], "rms_rel": dev[1]}}


def bench_brdf(eng, out, W=10000, NMU=16, NPHI=101, NF=8, n=3, slice_w=16):
    """ForwardModel_0.calc_brdf_matrix for a Hapke surface at the C4 size: W wavenumbers, NMU^2 (NPHI + 1) BRDF evaluations
    each.  Kernel time (hipEvents around the two launches), the call end to end (tables, staging, the matrix back to the
    host), and the NumPy restatement of tests/brdf_cases.py on the first 16 wavenumbers -- a SLICE, and NOT a comparator: the
    reference runs a numba-compiled point function under an interpreter loop, the restatement is vectorised NumPy."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import brdf_cases as bc
    rng = np.random.default_rng(7)
    P = bc.hapke_params(rng, W, 0.6)
    MU = bc.gauss_mu(NMU)
    wall = timeit(lambda: eng.brdf_matrix(2, P, MU, NPHI, NF), n)
    got = eng.brdf_matrix(2, P, MU, NPHI, NF)
    ms = eng.brdf_last()
    t = time.perf_counter()
    host = bc.brdf_matrix_np(2, P[:, :slice_w], MU, NPHI, NF)
    t_host = time.perf_counter() - t
    evals = W * NMU * NMU * (NPHI + 1)
    out["brdf_matrix_hapke_W%d_nmu%d_nphi%d_nf%d" % (W, NMU, NPHI, NF)] = {
        "kernel_ms": ms, "end_to_end_ms": 1e3 * wall, "hapke_evaluations": evals, "evaluations_per_s_kernel": evals / (1e-3 * ms),
        "matrix_bytes": int(got.nbytes), "numpy_restatement_s_on_a_slice_of_%d_wavenumbers" % slice_w: t_host,
        "slice_vs_gpu_rel_plane_max": bc.deviation(got[:slice_w], host)}


def bench_transit(eng, out, W=1024, n=5):
    """nemesisPTfm(gradients=True) at the C2 atmosphere as a transit (G = 20, S = 8, L = 100 -> P = 99 limb paths, LIMAX = 200,
    NPAR = 10, NPRO = 100, NX = 200): the fused call + map2pro + map2xvec on (W, NPAR, L, 1) beside the un-collapsed route --
    cirsradg_ck_transmission, map2pro and map2xvec on (W, NPAR, LIMAX, P), the trapezoid on the host -- alternated in one process,
    medians of n after one warm-up each.  `transit <W>`: another width; `transit <W> fused`: the fused route alone (W = 10000:
    the un-collapsed route would need 63 GB of device scratch) with its kernel times and the device memory it left reserved."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import transit_cases as tc
    from archnemesis_dist_amd import transit
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    fused_only = len(sys.argv) > 3 and sys.argv[3] == "fused"
    G, S, L, NP, NT, NPRO, NX = 20, 8, 100, 20, 15, 100, 200
    _, delg = syn.gauss_legendre_01(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S)
    free0 = torch.cuda.mem_get_info(0)[0]
    eng.upload_ktable(K, PRESS, TEMP, 200.0 + 0.1 * np.arange(W), delg); del K
    atm = syn.synth_atmosphere(L, S)
    rng = np.random.default_rng(4)
    NLAYIN, LAYINC, SCALE = tc.limb_paths(L, rng)
    SCALE = SCALE / 30.0
    BASEH = np.linspace(0.0, 4.0e5, L)
    RADIUS, RSTAR = 7.0e7, 7.0e5
    tan = transit.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    c = transit.path_weights(tan, RADIUS)
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    ig = np.arange(S, dtype=np.int32)
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    area_star = np.pi * (RSTAR * 1.0e3) ** 2
    P = NLAYIN.size

    def fused():
        AREA, _, _ = eng.cirsradg_ck_transit(lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE, c, gradients_on_device=True)
        eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L), DTE, DAM, DCO, to_host=False)
        d = eng.map2xvec(None, W, NVMR, NDUST, NPRO, 1, NX, xmap)
        return (AREA + np.pi * (RADIUS + tan[0] * 1.0e3) ** 2) / area_star * 100., d[:, 0, :] / area_star * 100.

    def uncollapsed():
        SPECOUT, dS = eng.cirsradg_ck_transmission(lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE)
        pro = eng.map2pro(dS, W, NVMR, NDUST, NPRO, P, NLAYIN, LAYINC, DTE, DAM, DCO)
        d = eng.map2xvec(pro, W, NVMR, NDUST, NPRO, P, NX, xmap)                     # (W, P, NX)
        return ((1. - SPECOUT) @ c + np.pi * (RADIUS + tan[0] * 1.0e3) ** 2) / area_star * 100., -np.einsum("wpx,p->wx", d, c) / area_star * 100.

    res = {"W": W, "G": G, "S": S, "L": L, "P": int(P), "NPAR": NPAR, "NPRO": NPRO, "NX": NX, "median_of": n}
    a = fused()
    tf, tu, kf, ku = [], [], [], []
    if not fused_only:
        b = uncollapsed()
        res["depth_max_rel_diff"] = float(np.max(np.abs(a[0] / b[0] - 1.0)))
        res["gradient_max_diff_over_max"] = float(np.max(np.abs(a[1] - b[1])) / np.max(np.abs(b[1])))
    for _ in range(n):
        t = time.perf_counter(); fused(); tf.append(time.perf_counter() - t)
        kf.append(eng.last_kernel_ms()["overlap_ms"])
        if not fused_only:
            t = time.perf_counter(); uncollapsed(); tu.append(time.perf_counter() - t)
            ku.append(eng.last_kernel_ms()["overlap_ms"])
    scratch, ms_sens, ms_grad = eng.transit_last()
    res.update(fused_wall_s=float(np.median(tf)), fused_overlapg_kernel_ms=float(np.median(kf)), k_transit_sens_ms=ms_sens,
               k_transit_grad_ms=ms_grad, transit_scratch_bytes=scratch,
               device_bytes_reserved_since_start=int(free0 - torch.cuda.mem_get_info(0)[0]))
    if not fused_only:
        res.update(uncollapsed_wall_s=float(np.median(tu)), uncollapsed_overlapg_kernel_ms=float(np.median(ku)),
                   overlapg_share_of_fused=float(np.median(kf)) * 1e-3 / float(np.median(tf)),
                   overlapg_share_of_uncollapsed=float(np.median(ku)) * 1e-3 / float(np.median(tu)))
    out["transit_C2_W%d" % W] = res


def bench_so(eng, out, W=1024, n=5):
    """nemesisSOfmg at the C2 atmosphere as a solar occultation (G = 20, S = 8, L = 100, Q = 10 tangent heights on the P = 20 limb
    paths that bracket them, LIMAX = 200, NPAR = 10, NPRO = 100, NX = 200): the fused call + map2pro + map2xvec on (W, NPAR, L, Q)
    beside the un-collapsed route -- cirsradg_ck_transmission, map2pro and map2xvec on (W, NPAR, LIMAX, P), the mix of the paths on
    the host -- alternated in one process, medians of n after one warm-up each.  `so <W>`: another width."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import occultation_cases as oc
    from archnemesis_dist_amd import occultation
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    G, S, L, Q, NP, NT, NPRO, NX = 20, 8, 100, 10, 20, 15, 100, 200
    _, delg = syn.gauss_legendre_01(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S)
    eng.upload_ktable(K, PRESS, TEMP, 200.0 + 0.1 * np.arange(W), delg); del K
    atm = syn.synth_atmosphere(L, S)
    rng = np.random.default_rng(4)
    NLAYIN, LAYINC, SCALE, bottoms = oc.occultation_paths(L, Q, rng)
    SCALE = SCALE / 30.0
    BASEH = np.linspace(0.0, 4.0e5, L)
    tan = occultation.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    TANHE = 0.5 * (tan[0::2] + tan[1::2]) + rng.uniform(-0.4, 0.4, Q) * (tan[1::2] - tan[0::2])
    C = occultation.tangent_mix(tan, TANHE)
    P = NLAYIN.size
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    ig = np.arange(S, dtype=np.int32)
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    nlay_q, layinc_q = np.array([L] * Q), np.ascontiguousarray(np.tile(np.arange(L)[:, None], (1, Q)))

    def fused():
        MOD, _, _ = eng.cirsradg_ck_occultation(lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE, C, gradients_on_device=True)
        eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlay_q, layinc_q, DTE, DAM, DCO, to_host=False)
        return MOD, eng.map2xvec(None, W, NVMR, NDUST, NPRO, Q, NX, xmap)

    def uncollapsed():
        SPECOUT, dS = eng.cirsradg_ck_transmission(lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE)
        pro = eng.map2pro(dS, W, NVMR, NDUST, NPRO, P, NLAYIN, LAYINC, DTE, DAM, DCO)
        d = eng.map2xvec(pro, W, NVMR, NDUST, NPRO, P, NX, xmap)                     # (W, P, NX)
        return SPECOUT @ C.T, np.einsum("wpx,qp->wqx", d, C)

    res = {"W": W, "G": G, "S": S, "L": L, "Q": Q, "P": int(P), "LIMAX": int(LAYINC.shape[0]), "NPAR": NPAR, "NPRO": NPRO, "NX": NX,
           "median_of": n, "entries_per_row_of_C": [int(v) for v in np.unique((C != 0).sum(axis=1))]}
    a, b = fused(), uncollapsed()
    res["spectrum_max_rel_diff"] = float(np.max(np.abs(a[0] / b[0] - 1.0)))
    res["gradient_max_diff_over_max"] = float(np.max(np.abs(a[1] - b[1])) / np.max(np.abs(b[1])))
    tf, tu, kf, ku = [], [], [], []
    for _ in range(n):
        t = time.perf_counter(); fused(); tf.append(time.perf_counter() - t)
        kf.append(eng.last_kernel_ms()["overlap_ms"])
        t = time.perf_counter(); uncollapsed(); tu.append(time.perf_counter() - t)
        ku.append(eng.last_kernel_ms()["overlap_ms"])
    fused()
    scratch, ms_paths, ms_grad = eng.occultation_last()
    res.update(fused_wall_s=float(np.median(tf)), fused_overlapg_kernel_ms=float(np.median(kf)), k_occ_paths_ms=ms_paths,
               k_occ_grad_ms=ms_grad, occultation_scratch_bytes=scratch, dMOD_bytes=8 * W * NPAR * L * Q,
               dSPECOUT_bytes=8 * W * NPAR * int(LAYINC.shape[0]) * int(P), uncollapsed_wall_s=float(np.median(tu)),
               uncollapsed_overlapg_kernel_ms=float(np.median(ku)))
    out["occultation_C2_W%d" % W] = res


def bench_limb(eng, out, W=1024, n=5):
    """nemesisLfmg at the C2 atmosphere as a limb observation, at the shape of the `so` mode (G = 20, S = 8, L = 100, Q = 10 tangent
    heights on the P = 20 limb paths that bracket them, LIMAX = 200, NPAR = 10, NPRO = 100, NX = 200, EMTEMP the layers'
    temperatures): the fused call + map2pro + map2xvec on (W, NPAR, L, Q) beside the un-collapsed device route --
    cirsradg_ck_thermal with dSPECOUT left on the device, map2pro and map2xvec on (W, NPAR, LIMAX, P), the mix of the paths on
    the host -- alternated in one process, medians (and extremes) of n after one warm-up each.  `limb <W>`: another width."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import occultation_cases as oc
    from archnemesis_dist_amd import limb
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    G, S, L, Q, NP, NT, NPRO, NX = 20, 8, 100, 10, 20, 15, 100, 200
    _, delg = syn.gauss_legendre_01(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S)
    eng.upload_ktable(K, PRESS, TEMP, 200.0 + 0.1 * np.arange(W), delg); del K
    atm = syn.synth_atmosphere(L, S)
    rng = np.random.default_rng(4)
    NLAYIN, LAYINC, SCALE, bottoms = oc.occultation_paths(L, Q, rng)
    SCALE = SCALE / 30.0
    BASEH = np.linspace(0.0, 4.0e5, L)
    tan = limb.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    TANHE = 0.5 * (tan[0::2] + tan[1::2]) + rng.uniform(-0.4, 0.4, Q) * (tan[1::2] - tan[0::2])
    C = limb.tangent_mix(tan, TANHE)
    P = NLAYIN.size
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    ig = np.arange(S, dtype=np.int32)
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    EMTEMP = np.where(np.arange(LAYINC.shape[0])[:, None] < NLAYIN[None, :], lt[LAYINC], 0.0)
    nlay_q, layinc_q = np.array([L] * Q), np.ascontiguousarray(np.tile(np.arange(L)[:, None], (1, Q)))

    def fused():
        MOD, _, _ = eng.cirsradg_ck_limb(0, lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE, EMTEMP, C,
                                         gradients_on_device=True)
        eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlay_q, layinc_q, DTE, DAM, DCO, to_host=False)
        return MOD, eng.map2xvec(None, W, NVMR, NDUST, NPRO, Q, NX, xmap)

    def uncollapsed():
        SPECOUT, _, _ = eng.cirsradg_ck_thermal(0, lp, lt, am, None, None, NVMR, NPAR, ig, NLAYIN, LAYINC, SCALE, EMTEMP, -1.0,
                                                gradients_on_device=True)
        eng.map2pro(None, W, NVMR, NDUST, NPRO, P, NLAYIN, LAYINC, DTE, DAM, DCO, to_host=False)
        d = eng.map2xvec(None, W, NVMR, NDUST, NPRO, P, NX, xmap)                    # (W, P, NX)
        return SPECOUT @ C.T, np.einsum("wpx,qp->wqx", d, C)

    res = {"W": W, "G": G, "S": S, "L": L, "Q": Q, "P": int(P), "LIMAX": int(LAYINC.shape[0]), "NPAR": NPAR, "NPRO": NPRO, "NX": NX,
           "median_of": n, "entries_per_row_of_C": [int(v) for v in np.unique((C != 0).sum(axis=1))]}
    a, b = fused(), uncollapsed()
    res["spectrum_max_rel_diff"] = float(np.max(np.abs(a[0] / b[0] - 1.0)))
    res["gradient_max_diff_over_max"] = float(np.max(np.abs(a[1] - b[1])) / np.max(np.abs(b[1])))
    tf, tu, kf, ku, rf, ru = [], [], [], [], [], []
    for _ in range(n):
        t = time.perf_counter(); fused(); tf.append(time.perf_counter() - t)
        k = eng.last_kernel_ms(); kf.append(k["overlap_ms"]); rf.append(k["rt_ms"])
        t = time.perf_counter(); uncollapsed(); tu.append(time.perf_counter() - t)
        k = eng.last_kernel_ms(); ku.append(k["overlap_ms"]); ru.append(k["rt_ms"])
    fused()
    scratch, ms_sens, ms_grad = eng.limb_last()
    res.update(fused_wall_s=float(np.median(tf)), fused_wall_s_min_max=[float(min(tf)), float(max(tf))],
               fused_overlapg_kernel_ms=float(np.median(kf)), fused_rt_ms=float(np.median(rf)), k_limb_planck_and_sens_ms=ms_sens,
               k_limb_grad_ms=ms_grad, limb_scratch_bytes=scratch, dMOD_bytes=8 * W * NPAR * L * Q,
               dSPECOUT_bytes=8 * W * NPAR * int(LAYINC.shape[0]) * int(P), uncollapsed_wall_s=float(np.median(tu)),
               uncollapsed_wall_s_min_max=[float(min(tu)), float(max(tu))], uncollapsed_overlapg_kernel_ms=float(np.median(ku)),
               uncollapsed_rt_ms=float(np.median(ru)))
    out["limb_C2_W%d" % W] = res


def bench_disc(eng, out, W=1024, n=5):
    """nemesisdiscfmg at the C2 atmosphere as one geometry of an unresolved planet (G = 20, S = 8, L = 100, NPAR = 10, NPRO = 100,
    NX = 200, a sequence from the top layer to the ground, EMTEMP the layers' temperatures) with NAV = 3 and 8 averaging points:
    the fused call + map2pro + map2xvec on (W, NPAR, L, 1) beside what runs without it -- NAV single-path cirsradg_ck_thermal
    calls with dSPECOUT brought to the host, the host maps (the CPU oracle's, standing in for the reference's) and the weighted
    sum -- alternated in one process, medians (and extremes) of n after one warm-up each.  Then k_disc_sens against k_limb_sens on
    the same paths: a sequence down to the bottom layer and up again (it does not reach the ground, as the limb entry requires).
    `disc <W>`: another width."""
    from oracle import oracle as orc
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    G, S, L, NP, NT, NPRO, NX = 20, 8, 100, 20, 15, 100, 200
    _, delg = syn.gauss_legendre_01(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S)
    eng.upload_ktable(K, PRESS, TEMP, 200.0 + 0.1 * np.arange(W), delg); del K
    atm = syn.synth_atmosphere(L, S)
    rng = np.random.default_rng(5)
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    ig = np.arange(S, dtype=np.int32)
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    deep_first = lp[0] > lp[-1]
    down = np.arange(L - 1, -1, -1) if deep_first else np.arange(L)             # from the top layer to the deepest
    nlay_1, layinc_1 = np.array([L]), np.arange(L)[:, None]
    for NAV in (3, 8):
        LAYINC = down.astype(np.int32)
        EMTEMP = lt[LAYINC]
        SCALE = np.ascontiguousarray(np.repeat((1.0 / np.cos(np.radians(np.linspace(0.0, 70.0, NAV))))[None, :], L, axis=0))
        C = rng.uniform(0.5, 1.0, (1, NAV)); C /= C.sum()

        def fused():
            MOD, _, dTS, _ = eng.cirsradg_ck_disc(0, lp, lt, am, None, None, NVMR, NPAR, ig, LAYINC, SCALE, EMTEMP, -1.0, mix=C,
                                                  gradients_on_device=True)
            eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, nlay_1, layinc_1, DTE, DAM, DCO, to_host=False)
            return MOD[:, 0], eng.map2xvec(None, W, NVMR, NDUST, NPRO, 1, NX, xmap)[:, 0, :]

        def point_by_point():
            spec, dspec = 0.0, 0.0
            for p in range(NAV):
                s1, d3, _ = eng.cirsradg_ck_thermal(0, lp, lt, am, None, None, NVMR, NPAR, ig, nlay_1, LAYINC[:, None],
                                                    SCALE[:, p:p + 1], EMTEMP[:, None], -1.0)
                d2 = orc.map2pro(d3, W, NVMR, NDUST, NPRO, 1, nlay_1, LAYINC[:, None], DTE, DAM, DCO)
                d1 = orc.map2xvec(d2, W, NVMR, NDUST, NPRO, 1, NX, xmap)
                spec = spec + C[0, p] * s1[:, 0]
                dspec = dspec + C[0, p] * d1[:, 0, :]
            return spec, dspec

        res = {"W": W, "G": G, "S": S, "L": L, "NAV": NAV, "N": int(L), "NPAR": NPAR, "NPRO": NPRO, "NX": NX, "median_of": n}
        a, b = fused(), point_by_point()
        res["spectrum_max_rel_diff"] = float(np.max(np.abs(a[0] / b[0] - 1.0)))
        res["gradient_max_diff_over_max"] = float(np.max(np.abs(a[1] - b[1])) / np.max(np.abs(b[1])))
        tf, tu, kf, ku = [], [], [], []
        for _ in range(n):
            t = time.perf_counter(); fused(); tf.append(time.perf_counter() - t)
            kf.append(eng.last_kernel_ms()["overlap_ms"])
            t = time.perf_counter(); point_by_point(); tu.append(time.perf_counter() - t)
            ku.append(eng.last_kernel_ms()["overlap_ms"])
        tc = []
        for _ in range(n):                                  # the fused call alone, without the maps
            t = time.perf_counter()
            eng.cirsradg_ck_disc(0, lp, lt, am, None, None, NVMR, NPAR, ig, LAYINC, SCALE, EMTEMP, -1.0, mix=C, gradients_on_device=True)
            tc.append(time.perf_counter() - t)
        scratch, ms_sens, ms_grad = eng.disc_last()
        res.update(fused_wall_s=float(np.median(tf)), fused_wall_s_min_max=[float(min(tf)), float(max(tf))],
                   fused_call_alone_wall_s=float(np.median(tc)), fused_overlapg_kernel_ms=float(np.median(kf)),
                   k_disc_planck_and_sens_ms=ms_sens, k_disc_grad_ms=ms_grad, disc_scratch_bytes=scratch, dMOD_bytes=8 * W * NPAR * L,
                   dSPECOUT_bytes_per_point=8 * W * NPAR * L, point_by_point_wall_s=float(np.median(tu)),
                   point_by_point_wall_s_min_max=[float(min(tu)), float(max(tu))],
                   point_by_point_overlapg_kernel_ms_per_call=float(np.median(ku)))
        # the same paths through both sensitivity kernels: down and up again, no ground
        LI2 = np.concatenate([LAYINC, LAYINC[::-1]]).astype(np.int32)
        SC2 = np.ascontiguousarray(np.concatenate([SCALE, SCALE[::-1]]))
        ET2 = lt[LI2]
        ms_d, ms_l = [], []
        for _ in range(n + 1):
            eng.cirsradg_ck_disc(0, lp, lt, am, None, None, NVMR, NPAR, ig, LI2, SC2, ET2, -1.0, mix=C, gradients_on_device=True)
            ms_d.append(eng.disc_last()[1])
            eng.cirsradg_ck_limb(0, lp, lt, am, None, None, NVMR, NPAR, ig, np.full(NAV, 2 * L, dtype=np.int32),
                                 np.ascontiguousarray(np.tile(LI2[:, None], (1, NAV))), SC2,
                                 np.ascontiguousarray(np.tile(ET2[:, None], (1, NAV))), C, gradients_on_device=True)
            ms_l.append(eng.limb_last()[1])
        res.update(down_and_up_k_disc_planck_and_sens_ms=float(np.median(ms_d[1:])),
                   down_and_up_k_limb_planck_and_sens_ms=float(np.median(ms_l[1:])))
        out["disc_C2_W%d_NAV%d" % (W, NAV)] = res


def bench_cia(eng, out, W=10000, n=5):
    """C3 (201 states through 100 profile levels, bench.py's table) with the CIA table of a synthetic H2 / He atmosphere: the
    numerical Jacobian with the continuum formed inside the batched call per distinct layer (fused), next to the same
    atmosphere without CIA (Rayleigh alone) and to CIA through calc_tau_cia over all layers and a dense taucont."""
    import torch
    import bench as B
    from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    dev = torch.device("cuda", eng.device)
    G, S, L, NP, NT = 20, 8, 100, 20, 15
    stream = torch.cuda.Stream(device=dev); torch.cuda.set_stream(stream)
    eng.set_stream(stream.cuda_stream)
    PRESS, TEMP, K = B.torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    WAVE = 200.0 + (1000.0 / W) * np.arange(W)
    eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
    pr = syn.synth_profiles(100, S + 2, seed=11)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2)])
    mk = lambda cia: BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)),
                                           layering_args=dict(NLAY=L, LAYINT=1, NINT=101), IRAY=4, cia=cia)

    def wall(model, reps):
        def f():
            torch.cuda.synchronize(); r = jacobian_nemesis_batched(model); torch.cuda.synchronize(); return r
        return timeit(f, reps), f()

    res = {"W": W, "G": G, "S": S, "L": L, "states": st.NX + 1}
    ray = mk(None)
    res["rayleigh_alone_s"], _ = wall(ray, n)
    res["rayleigh_alone_rows"] = list(ray.last_rows)
    model = mk(syn.synth_cia())
    res["cia_fused_s"], (YN, KK) = wall(model, n)
    res["cia_fused_rows"] = list(model.last_rows)
    model.fused_continuum = False
    res["cia_dense_s"], (YN_d, KK_d) = wall(model, 1)
    res["cia_dense_rows"] = list(model.last_rows)
    res["fused_equals_dense"] = bool(np.array_equal(YN, YN_d) and np.array_equal(KK, KK_d))
    res["median_of"] = n
    eng.set_stream(None)
    out["jacobian_C3_cia"] = res


def bench_grad_cont(eng, out, W=10000, n=5):
    """The gradient CIRSrad call of the analytic Jacobian at C3 size (one state, bench.py's table, 100 layers) with CIA, two
    aerosol populations and the Rayleigh continuum: the continuum and dTAUCON formed inside the call from the resident sources
    (cirsradg_ck_thermal_cont), next to the route it replaces -- calc_tau_cia(with_grad), calc_tau_dust, calc_tau_rayleigh, dTAUCON
    (W, NPAR, L) put together in NumPy and uploaded with cirsradg_ck_thermal.  Both leave dSPECOUT on the device, as
    jacobian_analytic does.  Wall times of host-pointer entries: PCIe staging included."""
    import torch
    import bench as B
    from archnemesis_dist_amd import layering
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    if len(sys.argv) > 2:
        W = int(sys.argv[2])
    dev = torch.device("cuda", eng.device)
    G, S, L, NP, NT, NDUST, IRAY = 20, 8, 100, 20, 15, 2, 4
    PRESS, TEMP, K = B.torch_ktable(torch, dev, W, G, NP, NT, S, seed=20260704)
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    WAVE = 200.0 + (1000.0 / W) * np.arange(W)
    eng.upload_ktable(K, PRESS.astype(np.float32), TEMP.astype(np.float32), WAVE, delg.astype(np.float32)); del K
    pr = syn.synth_profiles(100, S + 2, seed=11)
    NPRO, NVMR = pr["VMR"].shape
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2)])
    cia = syn.synth_cia()
    SWAVE = np.linspace(150.0, 1300.0, 12)
    x = np.linspace(0.0, 1.0, 12)[:, None]
    KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * x + np.arange(NDUST)[None])) * (1.0 + np.arange(NDUST)[None])
    KSCA = 0.7 * KEXT * (1.0 - 0.5 * x)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    model = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)),
                                  layering_args=dict(NLAY=L, LAYINT=1, NINT=101), IRAY=IRAY, cia=cia,
                                  dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST))
    res = {"W": W, "G": G, "S": S, "L": L, "NVMR": NVMR, "NDUST": NDUST, "IRAY": IRAY}
    res["jacobian_analytic_sources_s"] = timeit(lambda: model.jacobian_analytic(sources=True), n)
    lay = model.last_analytic_layers
    path = layering.calc_path(model.RADIUS, model.BASEH, lay["DELH"], lay["TEMP"], float(st.H[-1]), **model.geo)
    amount = np.ascontiguousarray(lay["AMOUNT"][:, model.igas_map].T) * 1.0e-4
    NPAR = NVMR + 2 + NDUST
    igas = model.igas_map.astype(np.int32)
    q = lay["PP"] / lay["PRESS"][:, None]
    f4 = eng.rayleigh_f4(pr["ID"], pr["ISO"], q)
    tabs = [cia[k] for k in ("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL",
                             "INORMALD")]
    rest = (NVMR, NPAR, igas, path.NLAYIN, path.LAYINC, path.SCALE, path.EMTEMP, -1.0)

    def fused():
        return eng.cirsradg_ck_thermal_cont(0, lay["PRESS"], lay["TEMP"], amount, q, lay["FRAC"], lay["TOTAM"], lay["DELH"], lay["CONT"],
                                            IRAY, f4, *rest, gradients_on_device=True)[0]

    def continuum():
        tcia, dcia = eng.calc_tau_cia(0, WAVE, *tabs, pr["ID"], pr["ISO"], lay["PP"], lay["PRESS"], lay["TEMP"], lay["FRAC"],
                                      lay["TOTAM"], lay["DELH"])
        dust4 = eng.calc_tau_dust(WAVE, SWAVE, KEXT, KSCA, lay["CONT"])
        ray, dray = eng.calc_tau_rayleigh(IRAY, 0, WAVE, lay["TOTAM"], ID=pr["ID"], ISO=pr["ISO"], VMR=q)
        cont = (tcia + np.sum(np.clip(np.nan_to_num(dust4[0]), 0, 1e20), 2)) + ray
        dcont = np.zeros((W, NPAR, L))                             # forward_model._ansfm_continuum
        dcont[:, 0:NVMR, :] += np.moveaxis(dcia[:, :, 0:NVMR], 2, 1) / lay["TOTAM"][None, None, :]
        dcont[:, NVMR, :] += dcia[:, :, NVMR]
        for i in range(NVMR):
            dcont[:, i, :] += dray
        for i in range(NDUST):
            dcont[:, NVMR + 1 + i, :] += dust4[2][:, :, i]
        return cont, dcont

    def host():
        cont, dcont = continuum()
        return eng.cirsradg_ck_thermal(0, lay["PRESS"], lay["TEMP"], amount, cont, dcont, *rest, gradients_on_device=True)[0]

    res["fused_entry_s"] = timeit(fused, n)
    res["host_assembled_route_s"] = timeit(host, n)
    res["host_continuum_and_assembly_s"] = timeit(continuum, n)
    res["dtaucon_bytes"] = 8 * W * NPAR * L
    res["same_spectrum_bits"] = bool(np.array_equal(fused(), host()))
    res["median_of"] = n
    out["grad_cont_C3"] = res


def bench_layer(eng, out):
    # ---- batched layering ---------------------------------------------------------------------------------------
    n, NPRO, V, D, NL = 201, 120, 8, 1, 100
    H = np.linspace(0, 6e5, NPRO); P = 1e6 * np.exp(-H / 3e4); T = 150 + 50 * np.sin(H / 1e5)
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0)
    VM = np.full((NPRO, V), 1e-4); DU = np.full((NPRO, D), 10.0)
    BH = np.linspace(0, 5.9e5, NL)
    t = timeit(lambda: eng.layer_average(7.1e7, rep(H), rep(P), rep(T), None, rep(VM), rep(DU), None, BH, None, LAYINT=1, NINT=101))
    out["layer_average_batch"] = {"wall_s": t, "states": n, "layers": NL, "nint": 101, "states_layers_per_s": n * NL / t}


if __name__ == "__main__":
    main()
