// cf_vah_coef.h -- the anisotropic-hydro 14-moment coefficients of DEVICE cells from the host (Lambda, alpha_L) tables, for entries outside
// cf_vah.hip (cf_sampler_vah.hip): cf_vah_coeffs, the kernel the spectra and the spacetime distributions run, with its table upload.
#pragma once
#include <stdint.h>

#include "../../include/is3d_amd.h"

namespace is3d {

// IS3D_EINVAL for tables that is3d_vah_coefficients refuses; no device use
int vah_tables_check(const is3d_vah_df_tables *tab);
// out[k][i] = c_k of cell i (n cells, Lambda in GeV); a cell beyond the last node gets zeros and atomicMin(status, cell0 + i).  Lambda, aL,
// out and status are DEVICE memory of the current device; the launch is on the null stream and has completed on return.
int vah_coeffs_device(const is3d_vah_df_tables *tab, int64_t n, int64_t cell0, const double *Lambda, const double *aL, double *const out[5],
                      unsigned long long *status);

}  // namespace is3d
