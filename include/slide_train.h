/*
 * slide_train.h -- C-ABI of the BACKWARD kernels of the row-major layers in libslide_hip.so (the
 * training step of the latent DDPMs).
 *
 * What they differentiate (reference, paths relative to /root/reference):
 *   MyGroupNorm + ReLU                       pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py:24-69
 *   grouping_operation / knn_gather (feats)  pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py:222-268, :506-507
 *                                            (the reference's native backward: _ext-src/src/group_points_gpu.cu:30-60)
 *   relu(cat([q.expand, k])), softmax over K + weighted sum    pointnet2_ops_lib/pointnet2_ops/attention.py:78-95
 * and whose forward counterparts are the module path's kernels (slide_engine.h: SLIDE_OP_ROWS_GN / _GROUP / _CONCAT_QK / _ATTN).
 * The reference gets these gradients from torch.autograd over ~80 module launches per forward (pointnet2/train.py,
 * pointnet2/train_latent_ddpm.py; losses: pointnet2/util.py:262-300, pointnet2/diffusion_utils/diffusion.py:319-341).
 *
 * All matrices are row-major fp32 [rows][ld] DEVICE arrays (ld = channels rounded up to 32, pad columns zero); outputs are
 * written in full unless stated.  Status: 0 = ok, else hipError_t (< 0: bad arguments).  Asynchronous on `stream`.
 */
#ifndef SLIDE_TRAIN_H
#define SLIDE_TRAIN_H

#include <stdint.h>

#include "slide_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y = post_relu?(GroupNorm_G(pre_relu?(x))) on [B*S][ld]: the first n_norm channels in G <= 64 groups over (group x S rows of a
 * sample), the rest pass through (MyGroupNorm); flags: 1 = ReLU before, 2 = ReLU after.  G = 0: no normalisation (ReLUs only;
 * gamma, beta, mean_rstd, dgamma, dbeta, scratch may be NULL).  mean_rstd [B][64][2]: the forward's statistics
 * (SLIDE_OP_ROWS_GN p[10], slide_engine.h).  Writes dx [B*S][ld] in full, pad columns included (there dx = dy, masked by x > 0
 * when a ReLU is set) and, with G > 0, the PER-SAMPLE parameter gradients dgamma, dbeta [B][ld] in full (zero beyond n_norm; the
 * caller sums over B: a deterministic reduction); with G = 0 dgamma and dbeta are not touched.  scratch: B * (64 * ld * 2 + 128)
 * floats.  B <= 0 or S <= 0: 0 without a launch.  -3, nothing written: ld not a positive multiple of 32 up to 1024, G outside
 * 0..64, n_norm outside 0..ld or no multiple of G, G = 0 with n_norm != 0, or G > 0 with a NULL among the six pointers above. */
SLIDE_API int slide_gn_rows_bwd(int B, int S, int ld, int G, int n_norm, int flags, const float *x, const float *gamma,
                                const float *beta, const float *mean_rstd, const float *dy, float *dx, float *dgamma, float *dbeta,
                                float *scratch, slide_stream_t stream);

/* out [ld] = column sums of x [rows][ld] (the bias gradient of a convolution: the sum of dy over the rows; GroupNorm's parameter
 * gradients over the batch); out is written in full (rows = 0: zeros).  rows < 128: one launch of 32-column stripes, scratch
 * unused (may be NULL).  rows >= 128: two launches, up to 1024 row chunks into scratch (1024 * ld floats), then 32-column stripes
 * over the partial rows.  Deterministic.  -3, nothing written: ld not a positive multiple of 32 up to 1024, rows < 0, or
 * rows >= 128 with scratch NULL. */
SLIDE_API int slide_col_sums(long long rows, int ld, const float *x, float *out, float *scratch, slide_stream_t stream);

/* out [B][ld] = the column sums of each sample's S rows of x [B*S][ld]: out[b][c] = sum_s x[(b, s)][c] (the gradient of a
 * per-sample vector added to every row of its sample -- the class- / t-embedding term of an Mlp); out is written in full.
 * Coalesced float4 row reads, no atomics, and a fixed order of additions that depends on S and ld only: a sample's sums do not
 * depend on B or on its position in the batch, and two runs are bit-equal.  S < 128: one launch, one workgroup per sample, scratch
 * unused (may be NULL).  S >= 128: two launches, n = min(256, S / 64) row chunks per sample into scratch (B * n * ld floats; never
 * more than B * 256 * ld), then the same kernel over each sample's partial rows.  gridDim.y = B: B <= 65535.  B = 0: 0 without a
 * launch, nothing read or written; S = 0 with B > 0: out zero-filled (a memset), no launch.  -3, nothing written: ld not a positive
 * multiple of 32 up to 1024, B < 0 or > 65535, S < 0, out NULL, x NULL with S > 0, or S >= 128 with scratch NULL. */
SLIDE_API int slide_col_sums_seg(int B, long long S, int ld, const float *x, float *out, float *scratch, slide_stream_t stream);

/* grouped rows out[(b,p,k)][0..C) = feat[b][idx[b][p][k]][0..C): dfeat [B*N][ldf] += dout [B*np*K][ldg] (atomic; dfeat must be
 * zero-initialised); counts (B*np) int32 or NULL: centres with count 0 carried zero features and receive nothing.  Only the
 * elements that a gradient row lands on are touched: channels >= C and rows that no live centre indexes keep their value. */
SLIDE_API int slide_group_rows_bwd(int B, int N, int np, int K, int C, int ldf, int ldg, const int64_t *idx, const int *counts,
                                   const float *dout, float *dfeat, slide_stream_t stream);

/* Backward of the COORDINATE columns of the grouped rows (SLIDE_OP_ROWS_GROUP; flags and column orders are the forward's):
 * dout [B*np*K][ldg] -> dxyz [B][N][3] (source points) and dnew_xyz [B][np][3] (centres); the reference differentiates them in
 * QueryAndGroup (pointnet2_utils.py:383-408) and group_knn (:506-520).  Row (b, p, k): q = xyz[b][idx[b][p][k]], c = new_xyz[b][p].
 *   SA form (flags & 1 == 0), columns C.. = rel, abs if flags & 2, centre if flags & 4:   dq += g_rel + g_abs,  dc += -g_rel + g_ctr
 *     (flags & 8: no coordinate columns, 0 without a launch)
 *   FP form (flags & 1), columns C.. = d2, w, abs(3), rel(3), centre(3); d2 [B][np][K] is the array the forward was given and is
 *     differentiated as |q - c|^2:  r_k = 1 / (d2_k + 1e-8), S = sum_k r_k, w_k = r_k / S,
 *     G_k = g_d2_k - (r_k^2 / S) (g_w_k - sum_j g_w_j w_j),  v_k = 2 G_k (q_k - c),
 *     dq_k += v_k + g_abs_k + g_rel_k,  dc += sum_k (-v_k - g_rel_k + g_ctr_k)
 * flags & 16: idx is int32, else int64.  counts (B*np int32) or NULL: a centre with count 0 was its own neighbour -- abs feeds dc,
 * rel contributes nothing, no source point is touched.
 * dnew_xyz is written in full, every element once, its K terms added in ascending k: deterministic, independent of the batch
 * position.  dxyz is ACCUMULATED with fp32 atomics (three per row) into a buffer the caller zeroes: not bit-reproducible.  Either
 * output may be NULL (not computed); both NULL: 0 without a launch.  B, N or np <= 0: 0 without a launch.  -3, nothing written: ld
 * not a positive multiple of 32 up to 1024, C < 0, C + the coordinate column count > ldg, K < 1, a NULL among xyz, new_xyz, idx,
 * dout, or the FP form with d2 NULL. */
SLIDE_API int slide_group_rows_coord_bwd(int B, int N, int np, int K, int C, int ldg, int flags, const float *xyz,
                                         const float *new_xyz, const void *idx, const float *d2, const int *counts, const float *dout,
                                         float *dxyz, float *dnew_xyz, slide_stream_t stream);

/* out = relu([q(point) broadcast over K | k(point, neighbour)]) with q [pts][ldq] (C1 channels), k [pts*K][ldk] (C2), out
 * [pts*K][ldo]: dq, dk from dout and the forward OUTPUT (the ReLU mask); the first C1 / C2 channels of dq / dk are written, their
 * pad columns are not touched (the caller zeroes them).  dk is a masked move; dq adds its K terms in ascending k: deterministic. */
SLIDE_API int slide_concat_qk_bwd(long long pts, int K, int C1, int ldq, int C2, int ldk, int ldo, const float *out,
                                  const float *dout, float *dq, float *dk, slide_stream_t stream);

/* out[pt][c] = sum_k softmax_k(s)[k][c] v[(pt,k)][c] over the first max(1, count) of the K neighbour rows (counts NULL: all K):
 * ds, dv [pts*K][lds | ldv] from s, v and dout [pts][ldo].  The first C channels of all K rows of a point are written: rows past
 * the count are WRITTEN as 0 in ds and dv; columns >= C are not touched (the caller zeroes them). */
SLIDE_API int slide_attn_rows_bwd(long long pts, int K, int C, int lds, int ldv, int ldo, const float *s, const float *v,
                                  const int *counts, const float *dout, float *ds, float *dv, slide_stream_t stream);

/* Backward of the fused Chamfer path (slide_hip.h Part 4: slide_chamfer_nn + slide_chamfer_reduce without lengths; feature term
 * `mse`, or none with f = 0) -- the reference's autoencoder loss, pointnet2/metrics_point_cloud/chamfer_and_f1.py:242-265.
 * x [b][n1][*], y [b][n2][*]: f32 rows of sx / sy >= 3 + f floats, xyz then f <= 16 feature channels; (d1, i1), (d2, i2): what
 * slide_chamfer_nn returned for (x, y); dred [b][2][5]: the gradient w.r.t. slide_chamfer_reduce's output (column 2, the F1 count,
 * is ignored).  Writes the dense gradients dx [b][n1][3 + f] and dy [b][n2][3 + f] in full; either may be NULL (not computed).
 * A point p of direction dir with neighbour q, squared distance d and feature term t = sum_c (fp_c - fq_c)^2 gives
 *   v = 2 (dred[dir][0] + dred[dir][1] / (2 sqrt d)) (p_xyz - q_xyz),  w = 2 (dred[dir][3] + dred[dir][4] / (2 sqrt t)) (fp - fq),
 * +v, +w to p and -v, -w to q.  CONVENTION: where d == 0 (t == 0) the square root's part is 0 -- the subgradient 0, where torch's
 * autograd yields NaN -- so the gradients are finite for all finite inputs.  Deterministic: every element is stored once, its
 * value the own-direction term and then the incoming terms in ascending source index (no atomics); a cloud's gradient does not
 * depend on its position in the batch.  b == 0: 0 without a launch; bad arguments (f, strides, NULL inputs): -2. */
SLIDE_API int slide_chamfer_cd_bwd(int b, int n1, int n2, int f, const float *x, int sx, const float *y, int sy, const float *d1,
                                   const int64_t *i1, const float *d2, const int64_t *i2, const float *dred, float *dx, float *dy,
                                   slide_stream_t stream);

/* The ENCODE side of autoencoder training (csrc/encoder_ops.hip).  Reference: the maxima of Pnet2Stage, pointnet2/models/pnet.py:32-40,
 * and DiagonalGaussianDistribution, pointnet2/data_utils/distributions.py:4-43, as pointnet2/models/point_upsample_decoder.py:96-147
 * applies it.  Common to the four: -3 with nothing written for a leading dimension that is not a positive multiple of 32 up to 1024,
 * B < 0, S < 0, S = 0 with B > 0, or a NULL among the pointers not marked optional; B = 0: 0 without a launch.  Inputs are finite;
 * NaN handling is not specified. */

/* out [B][ld], arg [B][ld] (int32): out[b][c] = max_s x[(b, s)][c] over the S >= 1 rows of sample b for c < C, arg[b][c] = the LOWEST
 * s that attains it (the first maximum in scan order: what max_pool2d's backward routes to).  Columns C..ld: out = 0, arg = -1.  One
 * workgroup per sample; a sample's result does not depend on B or on its position in the batch.  -3 also for C outside 0..ld. */
SLIDE_API int slide_col_max_seg(int B, int S, int C, int ld, const float *x, float *out, int *arg, slide_stream_t stream);

/* dx [B*S][ld], written in full: dx[(b, s)][c] = dy[b][c] where arg[b][c] == s, else 0 (arg = -1 in the pad columns: zeros).  A
 * gather: every element is stored once by the thread that owns it; no atomics, no zero fill. */
SLIDE_API int slide_col_max_seg_bwd(int B, int S, int ld, const int *arg, const float *dy, float *dx, slide_stream_t stream);

/* params [B*S][ldp]: mean in columns [0, C), log-variance in [C, 2C) (torch.chunk(parameters, 2, dim=1) of the reference's
 * channel-first tensor), 1 <= C, 2C <= ldp, C <= ldz.  lv = min(max(logvar, -30), 20).
 *   z [B*S][ldz]:  z[(b, s)][c] = mean + exp(0.5 lv) * eps[(b, s)][c] for c < C, 0 in columns C..ldz; eps [B*S][ldz], OPTIONAL:
 *                  NULL gives z = mean (the posterior's mode).  The kernel draws no numbers.
 *   kl [B], OPTIONAL (NULL: not computed):  kl[b] = 0.5 * sum over the sample's S x C elements of (mean^2 + exp(lv) - 1 - lv).
 * One workgroup of 256 threads per sample: thread t adds the terms of the elements t, t + 256, ... of the sample's S x ldz block in
 * ascending order, the 256 partial sums go through a fixed tree (a wave's xor butterfly 32, 16, .., 1, then the four wave sums in
 * ascending wave).  The order depends on S, C and ldz only: kl[b] is bit-equal over runs, over B and over the sample's position in
 * the batch.  exp is expf (1 ulp).  -3 also for S * ldz >= 2^31. */
SLIDE_API int slide_gauss_posterior_fwd(int B, int S, int C, int ldp, int ldz, const float *params, const float *eps, float *z,
                                        float *kl, slide_stream_t stream);

/* dparams [B*S][ldp], written in full (columns 2C..ldp zero), everything recomputed from params; dz [B*S][ldz] and dkl [B] are each
 * OPTIONAL (NULL: that term is 0), eps as in the forward (NULL: the dz term of dlogvar is 0):
 *   dmean   = dz + dkl[b] * mean
 *   dlogvar = m * (dz * eps * 0.5 * exp(0.5 lv) + dkl[b] * 0.5 * (exp(lv) - 1)),  m = 1 where -30 <= logvar <= 20, else 0
 * (torch.clamp's backward: the gradient passes AT both bounds). */
SLIDE_API int slide_gauss_posterior_bwd(int B, int S, int C, int ldp, int ldz, const float *params, const float *eps, const float *dz,
                                        const float *dkl, float *dparams, slide_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
