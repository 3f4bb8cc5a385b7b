// group_coord_bwd.hip -- gfx950 backward of the COORDINATE columns of the grouping kernel (rows_ops.hip rows_group_kernel): the
// gradient of a grouped matrix with respect to the source points xyz and the centres new_xyz.  The feature columns' backward is
// train_ops.hip group_rows_bwd_kernel; the two together differentiate QueryAndGroup (pointnet2_ops/pointnet2_utils.py:383-408) and
// group_knn (:506-520) for given neighbour indices.
//
// Row (b, p, k) with neighbour q = xyz[b][idx[b][p][k]] and centre c = new_xyz[b][p]; g_* = the row's incoming gradient columns.
//   SA  [rel = q - c | abs = q (flags & 2) | centre = c (flags & 4)]:
//         dq += g_rel + g_abs                  dc += -g_rel + g_ctr
//   FP  [d2 | w | abs | rel | centre], r_k = 1 / (d2_k + 1e-8), S = sum_k r_k, w_k = r_k / S, d2 differentiated as |q - c|^2:
//         G_k = g_d2_k - (r_k^2 / S) (g_w_k - sum_j g_w_j w_j)         v_k = 2 G_k (q_k - c)
//         dq_k += v_k + g_abs_k + g_rel_k      dc += -v_k - g_rel_k + g_ctr_k
//   a centre with an empty ball (counts == 0) was its own neighbour: abs feeds dc, rel and v vanish, no source point is touched.
//
// GC_G = 8 lanes own one centre: lane l takes the rows k = l, l + 8, ...  A row's three dq sums are formed in registers and leave as
// three fp32 atomics (dxyz: the scatter target, zeroed by the caller -- the contract of slide_group_rows_bwd).  The rows' dc terms
// are handed round the lane group and added in ASCENDING k by every lane, so dnew_xyz is stored once per element, without atomics:
// bit-reproducible and independent of the batch position.  S and sum_j g_w_j w_j are serial loops over the centre's K rows in every
// lane (S bit-equal to the forward's): no second launch, no scratch buffer.  Only the coordinate-gradient columns of dout are read.
// Compiled with -ffp-contract=off: every operation below rounds once (tests/group_coord_cases.py counts them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_train.h"
#include "launch.h"

namespace {

constexpr int GC_NT = 256;           // threads per workgroup
constexpr int GC_G = 8;              // lanes per centre
constexpr int GC_PTS = GC_NT / GC_G; // centres per workgroup

template <bool FP>
__global__ __launch_bounds__(GC_NT) void group_rows_coord_bwd_kernel(int N, int np, int K, int C, int ldg, int flags,
                                                                     const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                                     const void *__restrict__ idx, const float *__restrict__ d2,
                                                                     const int *__restrict__ counts, const float *__restrict__ dout,
                                                                     float *__restrict__ dxyz, float *__restrict__ dnew_xyz, size_t pts) {
  size_t pt = (size_t)blockIdx.x * GC_PTS + (threadIdx.x >> 3);  // b * np + p
  const int l = threadIdx.x & (GC_G - 1);
  const bool valid = pt < pts;  // (a lane group past the end keeps running on the last centre and stores nothing: the shuffles below
  if (!valid) pt = pts - 1;     //  stay convergent)
  const int b = (int)(pt / np);
  const bool empty = counts && counts[pt] == 0;
  const float *ctr = new_xyz + pt * 3;
  const float c[3] = {ctr[0], ctr[1], ctr[2]};
  const float *g0 = dout + pt * K * ldg + C;  // the coordinate-gradient columns of the centre's first row
  const bool has_abs = FP || (flags & 2), has_ctr = FP || (flags & 4);
  const int o_rel = FP ? 5 : 0, o_abs = FP ? 2 : 3, o_ctr = FP ? 8 : ((flags & 2) ? 6 : 3);

  float S = 0.f, T = 0.f;
  if (FP) {
    const float *dd = d2 + pt * K;
    for (int k = 0; k < K; ++k) S += 1.0f / (dd[k] + 1e-8f);
    for (int k = 0; k < K; ++k) T += g0[(size_t)k * ldg + 1] * ((1.0f / (dd[k] + 1e-8f)) / S);
  }

  float dc[3] = {0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += GC_G) {
    const int k = k0 + l;
    float tc[3] = {0.f, 0.f, 0.f};
    if (k < K) {
      const size_t row = pt * K + k;
      const float *g = g0 + (size_t)k * ldg;
      int nb = (flags & 16) ? static_cast<const int *>(idx)[row] : (int)static_cast<const int64_t *>(idx)[row];
      nb = nb < 0 ? 0 : (nb >= N ? N - 1 : nb);
      const size_t src = ((size_t)b * N + nb) * 3;
      float G2 = 0.f;
      if (FP) {
        const float r = 1.0f / (d2[row] + 1e-8f);
        G2 = 2.f * (g[0] - ((r * r) / S) * (g[1] - T));
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float g_rel = g[o_rel + j], g_abs = has_abs ? g[o_abs + j] : 0.f, g_ctr = has_ctr ? g[o_ctr + j] : 0.f;
        if (empty) {
          tc[j] = g_abs + g_ctr;
        } else {
          const float v = FP ? G2 * (xyz[src + j] - c[j]) : 0.f;
          tc[j] = (-v - g_rel) + g_ctr;
          if (dxyz && valid) atomicAdd(dxyz + src + j, (v + g_abs) + g_rel);
        }
      }
    }
    if (dnew_xyz) {
      const int nj = min(GC_G, K - k0);
      for (int u = 0; u < nj; ++u) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dc[j] += __shfl(tc[j], u, GC_G);
      }
    }
  }
  if (dnew_xyz && valid && l == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) dnew_xyz[pt * 3 + j] = dc[j];
  }
}

}  // namespace

extern "C" {

int slide_group_rows_coord_bwd(int B, int N, int np, int K, int C, int ldg, int flags, const float *xyz, const float *new_xyz,
                               const void *idx, const float *d2, const int *counts, const float *dout, float *dxyz, float *dnew_xyz,
                               slide_stream_t stream) {
  if (B <= 0 || N <= 0 || np <= 0) return 0;
  const bool fp = flags & 1;
  const int ncoord = fp ? 11 : (flags & 8) ? 0 : 3 + ((flags & 2) ? 3 : 0) + ((flags & 4) ? 3 : 0);
  if (ldg <= 0 || ldg % 32 || ldg > 1024 || C < 0 || C + ncoord > ldg || K < 1) return -3;
  if (!xyz || !new_xyz || !idx || !dout || (fp && !d2)) return -3;
  if (ncoord == 0 || (!dxyz && !dnew_xyz)) return 0;
  const size_t pts = (size_t)B * np;
  const dim3 grid((unsigned)((pts + GC_PTS - 1) / GC_PTS));
  if (fp)
    hipLaunchKernelGGL(group_rows_coord_bwd_kernel<true>, grid, dim3(GC_NT), 0, (hipStream_t)stream, N, np, K, C, ldg, flags, xyz,
                       new_xyz, idx, d2, counts, dout, dxyz, dnew_xyz, pts);
  else
    hipLaunchKernelGGL(group_rows_coord_bwd_kernel<false>, grid, dim3(GC_NT), 0, (hipStream_t)stream, N, np, K, C, ldg, flags, xyz,
                       new_xyz, idx, d2, counts, dout, dxyz, dnew_xyz, pts);
  return LAUNCH_STATUS();
}

}  // extern "C"
