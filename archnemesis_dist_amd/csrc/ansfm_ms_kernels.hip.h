// ansfm_ms_kernels.hip.h -- doubling/adding multiple-scattering core on gfx950.
//
// Restates Multiple_Scattering_Core.scloud11wave_core (Multiple_Scattering_Core.py:651-960) and its
// callees phasint2 :141, hansen :200, add :275, double1 :321, idown :366, addp :481, angle_quadrature :535,
// calc_rtj_matrix :566, for both viewing geometries (look-down: surface first, layers bottom to top; look-up: layers
// top to bottom, the surface kept apart and combined through idown when lowbc > 0).
//
// Decomposition (every (wavenumber, g, Fourier order) chain is independent):
//   k_ms_phase   one block per (wave, scatterer): azimuth-integrated phase matrices P++ / P+- for
//                ic = 0..nf.  They do not depend on g; the reference recomputes them inside its g
//                loop (:780-815) -- hoisted here.
//   k_ms_hansen_seq  Hansen renormalisation factors, sequential in the reference's (g, wave) order
//                (its fc array is carried from one iteration to the next, see the kernel).
//   k_ms_chain   one wavefront per (wave, g, ic): per layer doubling (double1/add) and adding
//                (addp) of the (R,T,J) operators, nmu x nmu float64 matrices in LDS; then the
//                2x2 (mu0,mu) samples of R u0+ + T u- + J for every path -> drad[wave][g][ic][path].
//   k_ms_chain16 the same chain for nmu == 16 with the stream x stream products on the matrix cores
//                (v_mfma_f64_16x16x4_f64), operands chained in the accumulator layout.
//   k_ms_fourier one thread per (wave, g, path): the Fourier sum with the reference's early-out
//                (:949-958) -> rad[path][g][wave].
//
// The units, in the order of a chain's life: ansfm_ms_params.h (parameter blocks), ansfm_ms_phase_kernels.hip.h,
// ansfm_ms_chain_kernels.hip.h, ansfm_ms_chain16_kernels.hip.h, ansfm_ms_optics_kernels.hip.h; ansfm_ms_lane.hip.h holds the
// one-lane-per-chain kernel and includes this file.
#pragma once
#include "ansfm_ms_params.h"
#include "ansfm_ms_phase_kernels.hip.h"
#include "ansfm_ms_chain_kernels.hip.h"
#include "ansfm_ms_chain16_kernels.hip.h"
#include "ansfm_ms_optics_kernels.hip.h"
