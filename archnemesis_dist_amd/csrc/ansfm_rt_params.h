// ansfm_rt_params.h -- arguments of the thermal / transmission / single-scattering RT kernels (ansfm_rt_kernels.hip.h) and of the
// transit kernels (ansfm_transit_kernels.hip.h).  The entry points fill them and ansfm_rt.hip / ansfm_transit.hip launch with
// them; no kernel and no device code here.
#pragma once
#include <stdint.h>

namespace ansfm {

struct RtParams {
    const double *tau;      // [n][L][G][Wpad], or [unique layers][G][Wpad] addressed through tau_slot
    const int32_t *tau_slot;// [n][L] row of tau holding layer (m, l), or nullptr (identity)
    const double *cont;     // [n][L][Wpad] or nullptr; cont_by_row: [rows][Wpad] addressed like tau
    const double *emi;      // [Li][Wpad] or nullptr  (array-level seam only)
    const double *wave;     // [W]
    const double *delg;     // [G]
    const int32_t *nlayin;  // [P]
    const int32_t *layinc;  // [LIMAX][P]
    const double *scale;    // [n][LIMAX][P]
    const double *emtemp;   // [n][LIMAX][P]
    const double *lay_press;// [n][L]  (Pa)
    const double *tsurf;    // [n]
    const double *emissivity, *solflux, *reflectance, *xfac;  // [W] or nullptr
    const double *sol_ang, *emiss_ang;                        // [P] or nullptr
    double *out;            // per_g ? [n][W][G] : [n][W][P]
    int W, Wpad, G, L, P, LIMAX, ispace, per_g;
    int mode;               // 0 thermal emission; 1 transmission exp(-sum tau) of the path (calculate_transmission_spectrum :4110);
                            // 2 single scattering, plane parallel (calc_singlescatt_plane_spectrum :6509-6600)
    // mode 2: single-scattering albedo of every layer, either given per g (array-level seam) or formed from the vertical
    // opacities as (TAURAY + TAUSCAT) / TAUTOT where TAUTOT > 0 (:4276-4283); layer-mean phase function per path; BRDF
    const double *omega;    // [Li][G][Wpad] along the path, or nullptr
    const double *sca;      // [n][L][Wpad] TAURAY + TAUSCAT of the layers, or nullptr
    const double *phase;    // [n][P][L][Wpad] (by layer; the array-level seam passes n = 1, L = Li, identity LAYINC)
    const double *brdf;     // [W][P] or nullptr
    // The states of a numerical Jacobian share the top of every path with state 0 (k_thermal_rt<.., PREFIX>): state 0's
    // launch (PREFIX 1, m0 = 0) leaves (taud, trold, spec) after every layer of the path in `prefix`
    // [P][LIMAX][3][G][Wpad]; the launch of the states m0 .. (PREFIX 2) starts state m's path ip at layer jstart[m][ip] --
    // the first one whose opacity row, continuum, SCALE or EMTEMP (mode 2 from the vertical opacities: or scattering opacity,
    // or phase function of that path) is not state 0's -- from that record.  Same bits.
    double *prefix;
    const int32_t *jstart;  // [n][P]
    int m0;
    int cont_by_row;
    // mode 2 on rows (ansfm_cirsrad_ck_singlescatt_batch_cont, the SS == 2 builds): sca [rows][Wpad] and phase [P][rows][Wpad]
    // addressed like tau; with cont_by_row (or no continuum) a layer is state 0's exactly when its row is
    int ss_by_row, rows;
};

constexpr int kMaxPar = 256;   // parameters of dSPECOUT (NVMR + 2 + NDUST): sizes the slot table in the kernel arguments only
struct RtGParams {
    RtParams r;              // r.out = SPECOUT [n][W][P]
    const double *dk;        // [n][L][NP1][G][Wpad]
    const double *dcont;     // [n][NPAR][L][Wpad] or nullptr   (dTAUCON)
    const double *dcont_gas; // [L][Wpad] or nullptr: one array added to the dTAUCON of EVERY gas parameter (kpar < NVMR) -- the
                             // Rayleigh term of calculate_layer_opacity (:3955-3957) without NVMR copies of it
    double *trold_ws;        // [n][P][LIMAX+1][G][Wpad]
    double *dspec;           // [n][P][NPAR][LIMAX][Wpad]   (internal layout)
    double *dtsurf;          // [n][W][P]
    int NPAR, NVMR, NP1;
    unsigned gas_mask;                    // as OverlapGParams::gas_mask: the slots of the other gases are zero and not read
    signed char slot_of_param[kMaxPar];   // -1 none, 0..S-1 gas slot (x1e-4), S = temperature slot
};

// Primary-transit depth with gradients (ansfm_transit_kernels.hip.h): the limb paths enter as the path matrix
// Sm[l][p] = sum of SCALE over the entries of path p that lie in layer l, compressed by path and by layer
struct TransitParams {
    const double *tau;       // [L][G][Wpad]
    const double *cont;      // [L][Wpad] or nullptr
    const double *delg;      // [G]
    const double *weight;    // [P] c_p: the annulus weight of path p in AREA = sum_p c_p (1 - T_p)
    const int32_t *col_ptr;  // [P + 1] entries of path p: col_ptr[p] .. col_ptr[p + 1]
    const int32_t *col_lay;  // [nnz] their layers
    const double *col_val;   // [nnz] Sm[l][p]
    const int32_t *row_ptr;  // [L + 1] entries of layer l
    const int32_t *row_path; // [nnz] their paths
    const double *row_val;   // [nnz] Sm[l][p]
    double *sens;            // [L][G][Wpad] A = sum_p c_p exp(-tau_path) Sm[l][p]
    double *tpart;           // [P][G][Wpad] exp(-tau_path) of every g-ordinate
    double *area;            // [W]
    double *trans;           // [W][P]
    double *darea;           // [W][NPAR][L]
    const double *dk;        // [L][NP1][G][Wpad]
    const double *dcont;     // [NPAR][L][Wpad] or nullptr
    const double *dcont_gas; // [L][Wpad] or nullptr (as RtGParams)
    int W, Wpad, G, L, P;
    int NPAR, NVMR, NP1;
    unsigned gas_mask;
    signed char slot_of_param[kMaxPar];
};
// rows of the 64-lane LDS tile of k_transit_sens that one workgroup may take (160 KiB / 512 B): the cap on layers and on paths
constexpr int kTransitMaxRows = 320;

}  // namespace ansfm
