#!/usr/bin/env python
"""Numerical Jacobian of a multiple-scattering forward model with respect to temperature and one aerosol profile at every
level -- no reference needed, synthetic table, atmosphere, CIA table and aerosols: NX + 1 forward models in ONE batched call
(jacobian_nemesis_batched on scatter_state.BatchedCKScatterModel).  CIA, aerosol extinction / scattering / fractions and
Rayleigh scattering are formed inside that call from sources resident on the GPU, once per distinct layer; layers that
equal the unperturbed state's are taken from its doubling results.

    python examples/c12_scatter_jacobian.py [NWAVE]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn
from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched
from archnemesis_dist_amd.profile_state import ContinuousProfileState
from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
G, S, L, NPRO, NMU, NF = 20, 6, 40, 40, 5, 2                      # 5 streams, Fourier orders 0 .. 2: the reference's defaults
eng = pkg.AnsfmEngine(0)
PRESS, TEMP, K = syn.synth_ktable(W, G, 20, 15, S, seed=1)
_, delg = syn.gauss_legendre_01(G)
WAVE = 200.0 + (1000.0 / W) * np.arange(W)
eng.upload_ktable(K, PRESS, TEMP, WAVE, delg); del K
pr = syn.synth_profiles(NPRO, S + 2, seed=2)
# two aerosol populations: a haze that thins out with height and a thin layer aloft (particles per m3 at the levels)
z = np.linspace(0.0, 1.0, NPRO)
DUST = np.stack([2.0e3 * np.exp(-4.0 * z), 3.0e2 * np.exp(-((z - 0.4) / 0.1) ** 2) + 1.0e-3], axis=1)
SWAVE = np.linspace(0.9 * WAVE[0], 1.1 * WAVE[-1], 12)
x = np.linspace(0.0, 1.0, 12)[:, None]
KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * x + np.arange(2)[None])) * (1.0 + np.arange(2)[None])
KSCA = 0.7 * KEXT * (1.0 - 0.5 * x)
# Henyey-Greenstein phase functions, tabulated (g = 0.6 and 0.3), as scloud11wave_core takes them: (NDUST, NWAVE, 2, NTHETA)
TH = np.linspace(0.0, 180.0, 41); c = np.cos(np.deg2rad(TH))
ph = np.zeros((2, W, 2, TH.size))
for d, g in enumerate((0.6, 0.3)):
    ph[d, :, 0, :] = ((1 - g * g) / (1 + g * g - 2 * g * c) ** 1.5 / (4 * np.pi))[None]
    ph[d, :, 1, :] = c[None]
ph = np.ascontiguousarray(ph[:, :, :, ::-1])
xq, wq = np.polynomial.legendre.leggauss(NMU)
MU, WTMU = 0.5 * (xq + 1.0), 0.5 * wq

state = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("DUST", 0)], DUST=DUST)
model = BatchedCKScatterModel(eng, state, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)), ph, MU, WTMU, NF, 101,
                              [30.0], [20.0], [45.0], np.full(W, 1.0e-8), layering_args=dict(NLAY=L, LAYINT=1, NINT=101), IRAY=4,
                              IMIE=1, cia=syn.synth_cia(), dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA))

jacobian_nemesis_batched(model)                                   # warm-up: buffers, the sources go up
t0 = time.perf_counter(); YN, KK = jacobian_nemesis_batched(model); t_fd = time.perf_counter() - t0
rows, total = model.last_rows
hits, layers = model.last_cache
print(f"state vector NX = {state.NX} (T and ln aerosol 0 at {NPRO} levels), spectrum NY = {YN.size}")
print(f"{state.NX + 1} forward models, {NMU} streams / NF {NF}: {t_fd * 1e3:7.1f} ms")
print(f"opacity and continuum rows computed: {rows} of {total};  layers from the first state's doubling results: {hits} of {layers}")
print("KK", KK.shape, " columns that are non-zero somewhere:", int(np.sum(np.any(KK != 0.0, axis=0))))
