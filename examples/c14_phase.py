#!/usr/bin/env python
"""The aerosol chain of a scattering forward model without a host step: a Mie population (Scatter_0.makephase) -> its double
Henyey-Greenstein fit (subfithgm) -> the phase function as a resident source of the engine (upload_phase, beside upload_dust)
-> the single-scattering and the multiple-scattering batch with the phase function formed in HBM
(cirsrad_ck_singlescatt_batch_src / cirsrad_ck_scatter_batch_src, through the model classes' phase_source=), on a synthetic
atmosphere.  Each result is compared with the same batch fed with the array read back from the source.

    python examples/c14_phase.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn
from archnemesis_dist_amd.jacobian import perturbed_states
from archnemesis_dist_amd.profile_state import ContinuousProfileState
from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel, BatchedCKSingleScatterModel


def main():
    eng = pkg.AnsfmEngine(0)
    W, G, S, NP, NT, NPRO, NLAY = 96, 8, 4, 8, 6, 20, 12
    # the table: wavenumbers 2000 .. 5000 cm-1
    WAVE = np.linspace(2000.0, 5000.0, W)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=1)
    _, delg = syn.gauss_legendre_01(G)
    eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)
    # one Mie population on six wavenumbers around the table's: cross sections and the fitted (f, g1, g2)
    SWAVE = np.linspace(1900.0, 5100.0, 6)
    wavel = 1.0e4 / SWAVE                                       # um
    refindx = np.tile([1.4, 0.01], (wavel.shape[0], 1))
    theta = np.linspace(0.0, 90.0, 21)
    rs = np.array([0.015 * wavel.min(), 0.0, 0.015 * wavel.min()])
    xscat, xext, thetax, phas = eng.mie_makephase(wavel, 2, np.array([0.5, 0.3, 0.0]), rs, refindx, theta)
    f, g1, g2, rms = eng.hg_fit(thetax, phas)
    print("double Henyey-Greenstein fit on %d wavenumbers: f %.3f .. %.3f  g1 %.3f .. %.3f  g2 %.3f .. %.3f"
          % (SWAVE.size, f.min(), f.max(), g1.min(), g1.max(), g2.min(), g2.max()))
    hg = np.array([f[:, None], g1[:, None], g2[:, None]])      # (3, NWAVE_scatter, NDUST = 1)
    dust = dict(SWAVE=SWAVE, KEXT=xext[:, None], KSCA=xscat[:, None])
    # the phase function at array level, then the atmosphere: temperature and the aerosol profile as the state
    print("calc_phase at 30 / 90 / 150 degrees, first wavenumber:", eng.calc_phase(0, SWAVE, None, hg, [30.0, 90.0, 150.0], WAVE)[0, :, 0],
          " Rayleigh:", eng.calc_phase_ray([30.0, 90.0, 150.0]))
    pr = syn.synth_profiles(NPRO, S + 2, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None]
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("DUST", 0)], DUST=DUST)
    st.calc_DSTEP()
    X = np.ascontiguousarray(perturbed_states(st.XN, st.DSTEP).T)[:5]
    args = (eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], list(range(2, S + 2)))
    la = dict(NLAY=NLAY, LAYINT=1, NINT=101)
    solar = np.full(W, 1.0e-8)

    # single scattering: phase_fn at the path's scattering angle, formed on the device
    kw = dict(layering_args=la, geometry=dict(ANGLE=20.0, EMISS_ANG=20.0), IRAY=1, dust=dust, BRDF=np.full((W, 1), 0.05))
    model = BatchedCKSingleScatterModel(*args, None, [30.0], [20.0], solar, phase_source=(0, None, hg), AZI_ANG=[45.0], **kw)
    Y = model.spectra_batch(X).cpu().numpy()
    alpha = eng.scattering_angle_deg([30.0], [20.0], [45.0])
    phase_fn = np.concatenate([eng.phase_from_source(alpha), np.broadcast_to(eng.calc_phase_ray(alpha)[None, :, None], (W, 1, 1))], axis=2)
    twin = BatchedCKSingleScatterModel(*args, phase_fn, [30.0], [20.0], solar, **kw)
    print("single scattering, %d states, scattering angle %.2f deg: radiance %.3e .. %.3e; equal to the batch fed from the host: %s"
          % (Y.shape[0], alpha[0], Y.min(), Y.max(), np.array_equal(twin.spectra_batch(X).cpu().numpy(), Y)))

    # multiple scattering, 5 streams: PHASE_ARRAY with (f, g1, g2) on the table's grid, formed on the device
    THETA = np.linspace(0.0, 180.0, 41)
    xq, wq = np.polynomial.legendre.leggauss(5)
    geo = (0.5 * (xq + 1.0), 0.5 * wq, 2, 101, [30.0], [20.0], [45.0], solar)
    kw = dict(layering_args=la, IRAY=1, IMIE=0, dust=dust)
    model = BatchedCKScatterModel(*args, None, *geo, phase_source=(0, THETA, hg), **kw)
    Y = model.spectra_batch(X).cpu().numpy()
    twin = BatchedCKScatterModel(*args, eng.phasarr_from_source(THETA), *geo, **kw)
    print("multiple scattering, %d states, 5 streams: radiance %.3e .. %.3e; equal to the batch fed from the host: %s"
          % (Y.shape[0], Y.min(), Y.max(), np.array_equal(twin.spectra_batch(X).cpu().numpy(), Y)))
    eng.close()


if __name__ == "__main__":
    main()
