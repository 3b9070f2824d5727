#!/usr/bin/env python
"""Numerical Jacobian of a single-scattering forward model (ISCAT = 3, plane parallel) with respect to temperature, one mixing
ratio and one aerosol profile at every level -- no reference needed, synthetic table, atmosphere, CIA table and aerosols: NX + 1
forward models in ONE batched call (jacobian_nemesis_batched on scatter_state.BatchedCKSingleScatterModel).  The continuum, the
scattering opacity and the layer-mean phase function of the path are formed inside that call from sources resident on the GPU,
once per distinct layer; every state starts the path from the record the unperturbed state left after the last layer the two
have in common.

    python examples/c13_singlescatt_jacobian.py [NWAVE]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn
from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched
from archnemesis_dist_amd.profile_state import ContinuousProfileState
from archnemesis_dist_amd.scatter_state import BatchedCKSingleScatterModel

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
G, S, L, NPRO = 20, 6, 40, 40
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
# the phase functions at the scattering angle of the one path: Henyey-Greenstein (g = 0.6 and 0.3) and, last, Rayleigh
SOL_ANG, EMISS_ANG, AZI_ANG = 30.0, 20.0, 45.0
rad = np.pi / 180.0
calpha = (np.sin(SOL_ANG * rad) * np.sin(EMISS_ANG * rad) * np.cos(AZI_ANG * rad - np.pi) - np.cos(EMISS_ANG * rad) * np.cos(SOL_ANG * rad))
hg = lambda g: (1 - g * g) / (1 + g * g - 2 * g * calpha) ** 1.5 / (4 * np.pi)
phase_fn = np.empty((W, 1, 3))
phase_fn[:, 0, :] = [hg(0.6), hg(0.3), 0.75 * (1.0 + calpha * calpha) / (4 * np.pi)]

state = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2), ("DUST", 0)], DUST=DUST)
model = BatchedCKSingleScatterModel(eng, state, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)), phase_fn, [SOL_ANG], [EMISS_ANG],
                                    np.full(W, 1.0e-8), layering_args=dict(NLAY=L, LAYINT=1, NINT=101),
                                    geometry=dict(ANGLE=EMISS_ANG, EMISS_ANG=EMISS_ANG), IRAY=1, cia=syn.synth_cia(),
                                    dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA), BRDF=np.full((W, 1), 0.05))

jacobian_nemesis_batched(model)                                   # warm-up: buffers, the sources go up
t0 = time.perf_counter(); YN, KK = jacobian_nemesis_batched(model); t_fd = time.perf_counter() - t0
rows, total = model.last_rows
print(f"state vector NX = {state.NX} (T, ln VMR 2 and ln aerosol 0 at {NPRO} levels), spectrum NY = {YN.size}")
print(f"{state.NX + 1} forward models, single scattering: {t_fd * 1e3:7.1f} ms")
print(f"opacity, continuum and phase rows computed: {rows} of {total};  paths started from the first state's records: {model.last_shared}")
print("KK", KK.shape, " columns that are non-zero somewhere:", int(np.sum(np.any(KK != 0.0, axis=0))))
