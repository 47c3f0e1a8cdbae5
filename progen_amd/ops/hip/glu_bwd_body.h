// One row-vector of the GLU-GELU backward, written once for glu_bwd_kernel
// (glu.hip) and glu_bwd_db_kernel (bias_grad.hip): thread i's 16 B vector of
// each half of row ``row``. The stored vectors come back in ``da_out`` / ``dg_out``
// for the caller that sums them; glu_bwd_kernel ignores them.
#pragma once

#include "common.h"

#define GLU_BLOCK 256

template <bool BF>
__device__ __forceinline__ void glu_bwd_row(const vec16_t<BF>* dy,
                                            const vec16_t<BF>* h,
                                            vec16_t<BF>* dh, long long row,
                                            int Hv, int i,
                                            vec16_t<BF>& da_out,
                                            vec16_t<BF>& dg_out) {
  using VEC = vec16_t<BF>;
  const VEC va = h[row * 2 * Hv + i];
  const VEC vg = h[row * 2 * Hv + Hv + i];
  const VEC vdy = dy[row * Hv + i];
  VEC da, dg;
#pragma unroll
  for (int j = 0; j < vec16<BF>::N; ++j) {
    const float d = vget<BF>(vdy, j);
    float gv, gg;
    gelu_tanh_both(vget<BF>(vg, j), &gv, &gg);
    vset<BF>(da, j, d * gv);
    vset<BF>(dg, j, d * vget<BF>(va, j) * gg);
  }
  dh[row * 2 * Hv + i] = da;
  dh[row * 2 * Hv + Hv + i] = dg;
  da_out = da;
  dg_out = dg;
}
