"""What the seven entries that form the continuum inside the call refuse about the nine arguments they share (use_cia, lay_q,
lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4): the return code of every refusal and the entry's name at the
head of ansfm_last_error.  Through the C-ABI, since the engine's methods refuse most of it in Python already.  Every call
returns before a pointer is read or a kernel is launched; the arrays are sound all the same (the _dev entries get device
tensors), so a call that were accepted would run inside them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, G, S, NP, NT = 5, 4, 1, 6, 5
N, L, P, LIMAX = 2, 3, 1, 3
NVMR, NDUST, NPAR = 3, 2, 3 + 2 + 2
NTH, NMU, NGEOM = 3, 4, 1
INVALID, NOTABLE, UNSUPPORTED = 1, 3, 5

# entry -> (the name its refusals of the shared arguments carry, the name in front of "upload a k-table first")
ENTRIES = {
    "thermal_cont_dev": ("cirsrad_ck_thermal_cont_dev", "cirsrad"),
    "grad_cont": ("cirsradg_ck_thermal_cont", "cirsradg"),
    "grad_cont_dev": ("cirsradg_ck_thermal_cont", "cirsradg"),
    "ss_cont": ("cirsrad_ck_singlescatt_batch_cont", "cirsrad_ck_singlescatt_batch_cont"),
    "ss_src": ("cirsrad_ck_singlescatt_batch_src", "cirsrad_ck_singlescatt_batch_src"),
    "ms_cont": ("cirsrad_ck_scatter_batch_cont", "cirsrad_ck_scatter_batch_cont"),
    "ms_src": ("cirsrad_ck_scatter_batch_src", "cirsrad_ck_scatter_batch_src"),
}
SINGLE_SCATTERING = ("ss_cont", "ss_src")
SCATTERING = ("ss_cont", "ss_src", "ms_cont", "ms_src")


def test_fused_continuum_refusals():
    import torch
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from test_continuum_fused_gpu import dust_table

    WAVE = 300.0 + 20.0 * np.arange(W)
    atm = syn.synth_atmosphere(L, S, seed=2, n_models=N)
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    ID, ISO = syn.PROFILE_GAS_ID[:NVMR].copy(), np.zeros(NVMR, dtype=np.int32)
    q = np.repeat(np.array([0.86, 0.13, 0.01])[None, None], N * L, 1).reshape(N, L, NVMR)
    host = dict(
        lp=atm["lay_press_pa"], lt=atm["lay_temp"], am=atm["amount"], q=q, frac=np.full((N, L), 0.25), totam=np.full((N, L), 1.0e24),
        delh=np.full((N, L), 20.0), cont=np.full((N, L, NDUST), 1.0e8), cont1=np.full((N, L, 1), 1.0e8), cont8=np.full((N, L, 8), 1.0e8),
        f4=np.full((N, L, 4), 0.25), NLAYIN=NLAYIN, LAYINC=LAYINC, SC=np.repeat(SCALE[None], N, 0),
        ET=np.ascontiguousarray(atm["lay_temp"][:, LAYINC[:, 0]][:, :, None]), ts=np.full(N, -1.0), spec=np.empty((N, W, P)),
        dspec=np.empty((N, W, NPAR, LIMAX, P)), dts=np.empty((N, W, P)))
    host = {k: np.ascontiguousarray(v) for k, v in host.items()}
    dev = {k: torch.as_tensor(v).cuda() for k, v in host.items()}
    ig = np.array([2], dtype=np.int32)                                       # a host array in every entry
    flux, ang, alpha = np.ones(W), np.zeros(P), np.full(P, 30.0)
    phase_fn = np.full((W, P, 9), 0.1)                                       # room for eight populations and Rayleigh
    theta = np.array([0.0, 90.0, 180.0]); mu_theta = np.cos(theta * np.pi / 180)
    phasarr = np.full((8, W, 2, NTH), 0.1)
    radg, solar, brdf = np.zeros((N, W, NMU)), np.ones(W), np.zeros((W, NMU, NMU, 1))
    mu1, wt1 = np.array([0.2, 0.4, 0.6, 0.8]), np.full(NMU, 0.25)
    geom = np.zeros(NGEOM)
    ms_spec = np.empty((N, W, NGEOM))

    def p(a):
        if a is None:
            return None
        return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    eng = pkg.AnsfmEngine(0)
    lib, ctx = eng._lib, eng._ctx

    def call(entry, use_cia=0, use_dust=0, ray_mode=0, ISPACE=0, ncont=None, cont="cont", drop=()):
        """one entry with the nine arguments as told: an array of a term that is on is given unless `drop` names it; ncont: the
        populations of use_dust"""
        a = dev if entry.endswith("_dev") else host
        g = lambda name, on: p(a[name]) if on and name not in drop else None
        nine = (use_cia, g("q", use_cia), g("frac", use_cia), g("totam", use_cia or ray_mode), g("delh", use_cia), use_dust,
                p(a[cont]) if use_dust and "cont" not in drop else None, ray_mode, g("f4", ray_mode == 4))
        ncont = (a[cont].shape[2] if use_dust else 0) if ncont is None else ncont
        head = (ctx, ISPACE, N, L, p(a["lp"]), p(a["lt"]), p(a["am"])) + nine
        path = (P, LIMAX, p(a["NLAYIN"]), p(a["LAYINC"]), p(a["SC"]), p(a["ET"]), p(a["ts"]))
        if entry == "thermal_cont_dev":
            return lib.ansfm_cirsrad_ck_thermal_cont_dev(*head, *path, None, None, None, None, None, None, p(a["spec"]))
        if entry in ("grad_cont", "grad_cont_dev"):
            fn = lib.ansfm_cirsradg_ck_thermal_cont if entry == "grad_cont" else lib.ansfm_cirsradg_ck_thermal_cont_dev
            return fn(*head, NVMR, NPAR, p(ig), *path, None, None, p(a["spec"]), p(a["dspec"]), p(a["dts"]))
        if entry in SINGLE_SCATTERING:
            fn = lib.ansfm_cirsrad_ck_singlescatt_batch_cont if entry == "ss_cont" else lib.ansfm_cirsrad_ck_singlescatt_batch_src
            return fn(*head, ncont, p(phase_fn if entry == "ss_cont" else alpha), *path, None, p(flux), p(flux), p(ang), p(ang), None,
                      p(a["spec"]))
        tail = (p(radg), NGEOM, p(geom), p(geom), p(geom), p(solar), 0, p(brdf), NMU, p(mu1), p(wt1), 0, 1, 0, 0, None, p(ms_spec), W, 0)
        if entry == "ms_cont":
            return lib.ansfm_cirsrad_ck_scatter_batch_cont(*head, ncont, NTH, p(phasarr), *tail)
        return lib.ansfm_cirsrad_ck_scatter_batch_src(*head, ncont, NTH, p(theta), p(mu_theta), *tail)

    seen = []

    def refused(what, entries, code, table=False, **kw):
        for e in entries:
            rc = call(e, **kw)
            msg = lib.ansfm_last_error(ctx).decode()
            seen.append((what, e, rc, msg))
            print(what, e, rc, msg)
            assert rc == code and msg.startswith(ENTRIES[e][1 if table else 0] + ":"), (what, e, rc, msg)

    every = tuple(ENTRIES)
    sound = dict(use_cia=1, use_dust=1, ray_mode=1)
    try:
        refused("no table", every, NOTABLE, table=True, **sound)
        _, delg = syn.gauss_legendre_01(G)
        PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=1)
        cia = lambda ISPACE: eng.upload_cia(ISPACE, WAVE, **syn.synth_cia(NWC=50, NT=4), ID=ID, ISO=ISO)
        # ---- a source that is not resident
        eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)
        eng.upload_dust(*dust_table(WAVE, NDUST))
        refused("use_cia before upload_cia", every, INVALID, **sound)
        eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)                        # a new table clears the sources
        cia(0)
        refused("use_dust before upload_dust", every, INVALID, use_dust=1, ray_mode=1)
        eng.upload_dust(*dust_table(WAVE, NDUST))
        # ---- both sources resident, CIA for ISPACE 0: one fault in the nine arguments
        refused("ray_mode = 3", every, INVALID, use_cia=1, use_dust=1, ray_mode=3)
        refused("ray_mode = 4, null f4", every, INVALID, use_cia=1, use_dust=1, ray_mode=4, drop=("f4",))
        refused("ray_mode = 1, null lay_totam", every, INVALID, use_dust=1, ray_mode=1, drop=("totam",))
        refused("use_cia, null lay_q", every, INVALID, drop=("q",), **sound)
        refused("use_cia, null lay_delh", every, INVALID, drop=("delh",), **sound)
        refused("use_dust, null lay_cont", every, INVALID, drop=("cont",), ncont=NDUST, **sound)
        refused("use_cia with ISPACE = 1", every, INVALID, ISPACE=1, **sound)
        refused("no term at all", every, INVALID)
        refused("use_cia alone", SINGLE_SCATTERING + ("ms_src",), INVALID, use_cia=1)
        refused("ncont = 1 against 2 populations", SCATTERING, INVALID, cont="cont1", **sound)
        # eight populations cannot be resident (ansfm_upload_dust refuses them), so ncont = 8 meets the two that are: the
        # single-scattering entries say UNSUPPORTED before they compare ncont with the source
        with pytest.raises(NotImplementedError, match="7"):
            eng.upload_dust(*dust_table(WAVE, 8))
        refused("ncont = 8", SINGLE_SCATTERING, UNSUPPORTED, cont="cont8", **sound)
        eng.synchronize()                                                    # the stream is sound after all of it
        assert len(seen) == 11 * 7 + 3 + 4 + 2
    finally:
        eng.close()
