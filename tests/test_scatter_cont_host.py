"""What the fused continuum of the scattering batch needs off the device: the entry ansfm_cirsrad_ck_scatter_batch_cont in the
header, the library and the engine; the aerosol block of ContinuousProfileState; the refusals of BatchedCKScatterModel."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ansfm_cirsrad_ck_scatter_batch_cont"


def _header_args(name):
    with open(os.path.join(ROOT, "include", "ansfm.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\s*\(([^()]*)\)\s*;", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_is_declared_exported_and_bound():
    import ctypes as C
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import _lib
    args = _header_args(ENTRY)
    assert ENTRY in _lib.EXPORTS
    restype, argtypes = _lib.PROTOTYPES[ENTRY]
    assert restype is C.c_int and len(argtypes) == len(args)
    # the rows entry's arguments without R, cont_row and the five row arrays, plus the continuum block of the thermal entry
    rows = _header_args("ansfm_cirsrad_ck_scatter_batch_rows")
    gone = {"int R", "const int32_t *cont_row", "const double *taucia_rows", "const double *taudust_rows", "const double *tauray_rows",
            "const double *tauscat_rows", "const double *lfrac_rows"}
    block = ["int use_cia", "const double *lay_q", "const double *lay_frac", "const double *lay_totam", "const double *lay_delh",
             "int use_dust", "const double *lay_cont", "int ray_mode", "const double *f4"]
    kept = [a for a in rows if a not in gone]
    assert len(kept) == len(rows) - 7 and sorted(args) == sorted(kept + block)
    assert args[-2:] == ["int W_full", "int w_begin"] and args.index("int use_cia") < args.index("int ray_mode") < args.index("int ncont")
    thermal = _header_args("ansfm_cirsrad_ck_thermal_cont_dev")
    i = thermal.index("int use_cia")
    assert thermal[i:i + len(block)] == block == args[args.index("int use_cia"):][:len(block)]
    for a, t in zip(args, argtypes):
        assert t is (C.c_void_p if "*" in a else C.c_int), a
    assert hasattr(_lib.load(), ENTRY)                          # the library exports it
    fn = pkg.AnsfmEngine.cirsrad_ck_scatter_batch_cont
    assert list(inspect.signature(fn).parameters)[:12] == ["self", "ISPACE", "lay_press_pa", "lay_temp", "amount", "q", "FRAC", "TOTAM",
                                                           "DELH", "CONT", "IRAY", "f4"]
    assert _lib.load().ansfm_abi_version() == 1


def _profiles(NPRO=7, NVMR=3, NDUST=2, seed=2):
    rng = np.random.default_rng(seed)
    H = np.linspace(0.0, 6.0e4, NPRO); P = 1.0e5 * np.exp(-H / 1.0e4); T = rng.uniform(100.0, 200.0, NPRO)
    VMR = rng.uniform(1e-6, 1e-2, (NPRO, NVMR)); DUST = rng.uniform(1.0, 1.0e3, (NPRO, NDUST))
    return H, P, T, VMR, DUST


def test_state_vector_with_an_aerosol_block_round_trip():
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    H, P, T, VMR, DUST = _profiles()
    NPRO = H.size
    st = ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 1), ("VMR", 2)], DUST=DUST)
    assert st.NX == 3 * NPRO and st.blocks == [("T", None), ("DUST", 1), ("VMR", 2)]
    assert np.array_equal(st.XN[:NPRO], T) and np.array_equal(st.XN[NPRO:2 * NPRO], np.log(DUST[:, 1]))
    assert np.array_equal(st.XN[2 * NPRO:], np.log(VMR[:, 2]))
    out = st.profiles(st.XN)
    assert len(out) == 3
    T1, VMR1, DUST1 = out
    assert T1.shape == (1, NPRO) and VMR1.shape == (1,) + VMR.shape and DUST1.shape == (1,) + DUST.shape
    assert np.array_equal(T1[0], T) and np.array_equal(DUST1[0, :, 0], DUST[:, 0]) and np.array_equal(VMR1[0, :, :2], VMR[:, :2])
    assert np.array_equal(DUST1[0, :, 1], np.exp(np.log(DUST[:, 1])))                   # un-logged, as subprofretg un-logs it
    np.testing.assert_allclose(DUST1[0, :, 1], DUST[:, 1], rtol=4e-16)                  # exp(log x) = x to an ulp or two
    X = np.repeat(st.XN[None], 3, 0)
    X[1, NPRO + 4] += 0.05; X[2, 2] += 1.0
    T3, VMR3, DUST3 = st.profiles(X)
    assert np.array_equal(DUST3[0], DUST1[0]) and np.array_equal(DUST3[2], DUST1[0])
    assert DUST3[1, 4, 1] == np.exp(np.log(DUST[4, 1]) + 0.05) and np.array_equal(np.delete(DUST3[1], 4, 0), np.delete(DUST1[0], 4, 0))
    assert T3[2, 2] == T[2] + 1.0
    assert np.array_equal(st.calc_DSTEP(), 0.05 * st.XN)
    with pytest.raises(ValueError):
        ContinuousProfileState(H, P, T, VMR, [("DUST", 0)])                             # no DUST given
    with pytest.raises(ValueError):
        ContinuousProfileState(H, P, T, VMR, [("DUST", 2)], DUST=DUST)                  # no such column
    with pytest.raises(ValueError):
        ContinuousProfileState(H, P, T, VMR, [("CLOUD", 0)], DUST=DUST)


def test_state_vector_without_an_aerosol_block_is_unchanged():
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    H, P, T, VMR, DUST = _profiles()
    NPRO = H.size
    for extra in ({}, {"DUST": DUST}):                          # DUST given, no block: still two values
        st = ContinuousProfileState(H, P, T, VMR, ["T", ("VMR", 1)], **extra)
        assert st.NX == 2 * NPRO and st.blocks == [("T", None), ("VMR", 1)]
        assert np.array_equal(st.XN, np.concatenate([T, np.log(VMR[:, 1])]))
        out = st.profiles(np.stack([st.XN, st.XN + 0.1]))
        assert isinstance(out, tuple) and len(out) == 2
        T2, VMR2 = out
        assert np.array_equal(T2[0], T) and np.array_equal(T2[1], T + 0.1)
        want = VMR.copy(); want[:, 1] = np.exp(np.log(VMR[:, 1]) + 0.1)
        assert np.array_equal(VMR2[1], want)
    # the thermal model does not know the block
    st = ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=DUST)
    with pytest.raises(NotImplementedError):
        BatchedCKThermalModel(None, st, 7.0e7, [39, 40, 6], [0, 0, 0], [2])


def test_scatter_model_refusals_need_no_device():
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel
    H, P, T, VMR, _ = _profiles()
    NPRO = H.size
    mk = lambda st, **kw: BatchedCKScatterModel(None, st, 7.0e7, [39, 40, 6], [0, 0, 0], [2], None, np.ones(5), np.ones(5), 2, 101, [30.0],
                                                [20.0], [0.0], np.ones(4), **kw)
    D8 = np.ones((NPRO, 8))
    K8 = dict(SWAVE=np.linspace(1.0, 2.0, 4), KEXT=np.ones((4, 8)), KSCA=np.ones((4, 8)))
    with pytest.raises(NotImplementedError, match="7"):
        mk(ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D8), dust=K8)
    with pytest.raises(NotImplementedError, match="7"):
        mk(ContinuousProfileState(H, P, T, VMR, ["T"]), dust=dict(K8, DUST=D8))
    D2 = np.ones((NPRO, 2))
    K2 = dict(SWAVE=np.linspace(1.0, 2.0, 4), KEXT=np.ones((4, 2)), KSCA=np.ones((4, 2)))
    with pytest.raises(NotImplementedError, match="DUST_RENORMALISATION"):
        mk(ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), dust=K2, DUST_RENORMALISATION=True)
    with pytest.raises(ValueError):                             # a DUST block without the cross sections
        mk(ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2))
    with pytest.raises(ValueError):                             # cross sections of three populations, profiles of two
        mk(ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), dust=dict(K2, KEXT=np.ones((4, 3)), KSCA=np.ones((4, 3))))
