/*
 * slide_hip.h -- C-ABI of libslide_hip.so (hand-written gfx950 HIP kernels).
 *
 * Part 1 is the drop-in boundary of the reference's native extension `pointnet2_ops._ext`:
 * one entry point per reference `*_kernel_wrapper`, SAME name, SAME argument order and meaning,
 * plus a trailing stream and an int status (0 = ok, otherwise the hipError_t; the reference
 * prints and exit(-1)s instead, _ext-src/include/cuda_utils.h:30-39).  Reference prototypes
 * (paths relative to pointnet2_ops_lib/pointnet2_ops/_ext-src/):
 *   src/sampling.cpp:4-13      gather_points[_grad]_kernel_wrapper, furthest_point_sampling_kernel_wrapper
 *   src/ball_query.cpp:6-8     query_ball_point_kernel_wrapper
 *   src/group_points.cpp:4-10  group_points[_grad]_kernel_wrapper
 *   src/interpolate.cpp:4-12   three_nn_kernel_wrapper, three_interpolate[_grad]_kernel_wrapper
 * All pointers are DEVICE pointers to contiguous fp32 / int32 arrays; outputs are allocated and
 * initialised by the caller exactly like the reference host code does (zeros; FPS `temp` = 1e10).
 * Kernels are asynchronous on `stream` (a hipStream_t passed as void*); no host sync.
 *
 * Part 2 adds what the executed configs need from un-vendored pytorch3d 0.7.0 (knn_points /
 * knn_gather, call sites pointnet2_ops/pointnet2_utils.py:370,506-507).
 *
 * Part 4 is the Chamfer / F1 metric (the reference's pointnet2/metrics_point_cloud/chamfer_and_f1.py, forward only).
 *
 * Part 5 is DPSR, oriented points to the Poisson indicator grid (the reference's pointnet2/dpsr_utils/dpsr.py), forward and backward.
 *
 * Part 6 is marching cubes, the indicator grid to an indexed triangle mesh (the reference calls skimage.measure.marching_cubes on the
 * host: pointnet2/dpsr_utils/utils.py mc_from_psr).
 *
 * Part 8 is mesh clean-up: connected components of a batch of triangle meshes and the keep-largest filter (the reference's
 * verts_on_largest_mesh in the same file, igl and trimesh on the host).
 *
 * Part 9 is the refine-and-upsample front of DPSR: mirror and tag a cloud, split every point into its children, normalise and clamp
 * them into DPSR's cube (the reference's data_utils/mirror_partial.py, models/point_upsample_module.py and the tail of
 * network_output_to_dpsr_grid), bit for bit.
 *
 * Part 3 is the fused latent-DDPM denoiser engine (the reference runs these as ~80 torch module
 * launches per step: pointnet2/models/pointnet2_with_pcld_condition.py:286-489).
 */
#ifndef SLIDE_HIP_H
#define SLIDE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *slide_stream_t; /* hipStream_t */
#define SLIDE_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------ Part 1: pointnet2_ops._ext */
/* sampling.cpp:4-6   points (b,c,n) f32, idx (b,npoints) i32 -> out (b,c,npoints) */
SLIDE_API int gather_points_kernel_wrapper(int b, int c, int n, int npoints, const float *points,
                                 const int *idx, float *out, slide_stream_t stream);
/* sampling.cpp:7-9   grad_out (b,c,npoints) -> grad_points (b,c,n) += (caller zero-fills) */
SLIDE_API int gather_points_grad_kernel_wrapper(int b, int c, int n, int npoints, const float *grad_out,
                                      const int *idx, float *grad_points, slide_stream_t stream);
/* sampling.cpp:11-13 dataset (b,n,3), temp (b,n) pre-filled 1e10 (updated in place), idxs (b,m) */
SLIDE_API int furthest_point_sampling_kernel_wrapper(int b, int n, int m, const float *dataset, float *temp,
                                           int *idxs, slide_stream_t stream);
/* ball_query.cpp:6-8 new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample), counts (b,m); both zero-filled */
SLIDE_API int query_ball_point_kernel_wrapper(int b, int n, int m, float radius, int nsample,
                                    const float *new_xyz, const float *xyz, int *idx, int *counts,
                                    slide_stream_t stream);
/* group_points.cpp:4-6  points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample) */
SLIDE_API int group_points_kernel_wrapper(int b, int c, int n, int npoints, int nsample, const float *points,
                                const int *idx, float *out, slide_stream_t stream);
/* group_points.cpp:8-10 */
SLIDE_API int group_points_grad_kernel_wrapper(int b, int c, int n, int npoints, int nsample,
                                     const float *grad_out, const int *idx, float *grad_points,
                                     slide_stream_t stream);
/* interpolate.cpp:4-5   unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3), idx (b,n,3) */
SLIDE_API int three_nn_kernel_wrapper(int b, int n, int m, const float *unknown, const float *known,
                            float *dist2, int *idx, slide_stream_t stream);
/* interpolate.cpp:6-8   points (b,c,m), idx (b,n,3), weight (b,n,3) -> out (b,c,n) */
SLIDE_API int three_interpolate_kernel_wrapper(int b, int c, int m, int n, const float *points, const int *idx,
                                     const float *weight, float *out, slide_stream_t stream);
/* interpolate.cpp:9-12  grad_out (b,c,n) -> grad_points (b,c,m) += */
SLIDE_API int three_interpolate_grad_kernel_wrapper(int b, int c, int n, int m, const float *grad_out,
                                          const int *idx, const float *weight, float *grad_points,
                                          slide_stream_t stream);

/* ------------------------------------------------------------------ Part 2: pytorch3d.ops.knn */
/* p1 (b,n1,3), p2 (b,n2,3), lengths2 (b) int64 or NULL -> dists (b,n1,K) f32 ascending squared L2,
 * idx (b,n1,K) int64; ties -> lower index; K <= 64 (returns -2 beyond).  Slots beyond lengths2 stay (0, 0). */
SLIDE_API int slide_knn_points(int b, int n1, int n2, int K, const float *p1, const float *p2,
                     const int64_t *lengths2, float *dists, int64_t *idx, slide_stream_t stream);
/* x (b,n2,u), idx (b,n1,K) int64 -> out (b,n1,K,u) */
SLIDE_API int slide_knn_gather(int b, int n2, int u, int n1, int K, const float *x, const int64_t *idx,
                     float *out, slide_stream_t stream);

/* pytorch3d.ops.sample_farthest_points (call site pointnet2/models/point_upsample_decoder.py:178-180): plain iterative
 * FPS without the near-origin skip; start_idx (b) int32 in [0, n) (clamped to it) or NULL (= 0); temp (b,n) pre-filled 1e10; idx (b,K) int32;
 * ties -> lowest index. */
SLIDE_API int slide_sample_farthest_points(int b, int n, int K, const float *points, const int *start_idx, float *temp,
                                           int *idx, slide_stream_t stream);

/* Row-layout gather (build addition; the (B, N, C) counterpart of gather_points, sampling.cpp:4-6): points (b,n,c) row-major,
 * idx (b,m) int32 -> out (b,m,c).  Moves exactly the gathered bytes; gather_points' (B,C,N) layout costs a 64-byte sector per
 * gathered element.  What FPS -> gather of the row-major module path and of (B,N,3) coordinates uses. */
SLIDE_API int slide_gather_rows(int b, int n, int m, int c, const float *points, const int *idx, float *out,
                                slide_stream_t stream);

/* ------------------------------------------------------------------ Part 4: Chamfer / F1 metric */
/* Bidirectional nearest neighbour (K = 1) of a batch of cloud pairs.  x (b,n1,sx) / y (b,n2,sy) f32 row-major, xyz = the first three
 * floats of every point (sx, sy >= 3: a (B,N,C) tensor with features behind xyz is read in place); x_lengths / y_lengths (b) int64
 * in [1, n] or NULL (= n).  -> d1 (b,n1) f32 squared L2 distance of each valid point of x to its nearest valid point of y, i1 (b,n1)
 * int64 that point's index; d2 / i2 the other direction.  Bit-equal to slide_knn_points(K = 1) (ties -> lower index); slots beyond a
 * cloud's length hold (0, 0).  Returns -2 for sx or sy < 3. */
SLIDE_API int slide_chamfer_nn(int b, int n1, int n2, const float *x, int sx, const float *y, int sy, const int64_t *x_lengths,
                               const int64_t *y_lengths, float *d1, int64_t *i1, float *d2, int64_t *i2, slide_stream_t stream);
/* Per-cloud reductions of slide_chamfer_nn's output over the valid points, in a fixed order (a pair's results do not depend on its
 * batch): out (b,2,5) f32, [pair][direction] = { sum d, sum sqrt d, count of d < threshold, sum term, sum sqrt term }.  term =
 * the normal term between a point's features and its nearest neighbour's: mode 0 none (i1 / i2 / fx / fy may be NULL, the last two
 * sums are 0), 1 mse sum_c (f - f_nn)^2, 2 cos 1 - |cosine_similarity(f, f_nn, eps = 1e-6)|.  fx (b,n1,sfx) / fy (b,n2,sfy): F
 * channels per point at a row stride of sfx / sfy floats.  Returns -2 for an invalid mode / F / stride. */
SLIDE_API int slide_chamfer_reduce(int b, int n1, int n2, const float *d1, const int64_t *i1, const float *d2, const int64_t *i2,
                                   const int64_t *x_lengths, const int64_t *y_lengths, float threshold, int F, int mode,
                                   const float *fx, int sfx, const float *fy, int sfy, float *out, slide_stream_t stream);
/* All-pairs Chamfer sums of two SETS of fixed-size clouds, one launch: x (m,p,sx) / y (n,q,sy) f32 row-major, xyz = the first three
 * floats of every point (sx, sy >= 3) -> out (m,n,2,2) f32, out[i][j][0] = { sum, sum of square roots } over the points of x[i] of
 * the squared L2 distance to the nearest point of y[j], out[i][j][1] the same over the points of y[j] towards x[i].  Every entry is
 * bit-equal to columns 0 and 1 of slide_chamfer_reduce(slide_chamfer_nn(x[i], y[j])) and does not depend on m, n, the pair's
 * position or `symmetric`.  symmetric = 1: y is x (m == n, p == q); the upper triangle and the diagonal are computed, the lower
 * triangle is their mirror out[j][i][d] = out[i][j][1 - d].  Returns -2 for sx or sy < 3, for symmetric with m != n or p != q and
 * for more than 2^31 - 1 workgroups (8 * ceil(n / 8) * m); 0 without a launch when m, n, p or q is 0. */
SLIDE_API int slide_chamfer_pairwise(int m, int n, int p, int q, const float *x, int sx, const float *y, int sy, int symmetric,
                                     float *out, slide_stream_t stream);
/* All-pairs approximate Earth Mover's Distance of two SETS of fixed-size clouds (the reference's PyTorchEMD approxmatch + matchcost,
 * forward only), one launch: x (m,p,sx) / y (n,q,sy) f32 row-major, xyz = the first three floats of every point (sx, sy >= 3) ->
 * out (m,n) f32, out[i][j] = the RAW cost sum_kl d(k,l) match(k,l) with x[i] as xyz1 (p points) and y[j] as xyz2 (q points), d the
 * squared L2 distance: ten levels exp(-4^7 d) ... exp(-d / 4), 1 of the auction written out in csrc/emd_pairwise.hip; the match
 * itself is never stored.  Not divided by a point count (the PVD metric divides by p).  NOT symmetric in its arguments:
 * out(x, y) is not the transpose of out(y, x), so a set against itself is computed in full.  paired != 0: m == n is required and
 * only the m pairs (i, i) are computed, out (m), out[i] = cost(x[i], y[i]).  One workgroup per ordered pair, no atomics: an entry
 * depends on its two clouds only -- not on m, n, the pair's position or the form that computed it.  The pair's mass vectors live
 * in LDS, in double while they fit (p + q <= 9600), in float beyond (p + q <= 19456; p = q = 8192 fits).  Returns -2 for sx or sy < 3, for paired
 * with m != n, for clouds beyond that limit and for more than 2^31 - 1 workgroups (8 * ceil(n / 8) * m); 0 without a launch when
 * m, n, p or q is 0. */
SLIDE_API int slide_emd_pairwise(int m, int n, int p, int q, const float *x, int sx, const float *y, int sy, int paired, float *out,
                                 slide_stream_t stream);

/* Occupancy counters of S clouds of P points on an R^3 lattice (the JSD metric's grid_counters / grid_bernoulli_rvars), one launch.
 * pts (s,p,sp) f32 row-major, xyz = the first three floats of a point (sp >= 3); axis (r) f32, the strictly ascending cell-centre
 * coordinates of one axis (cell (i,j,k) = (axis[i], axis[j], axis[k]), flat index (i r + j) r + k); rowmask (r*r) uint32, bit k of
 * word i r + j set when cell (i,j,k) is admissible; 2 <= r <= 32.  Every point goes to the admissible cell with the smallest fp32
 * squared distance fmaf(dz, dz, fmaf(dy, dy, dx * dx)), exact ties to the lowest flat index (the two-step rule is written out in
 * csrc/occupancy_grid.hip).  ACCUMULATED into (the caller zero-fills): counts (r^3) int32 += points per cell, clouds (r^3) int32 +=
 * clouds with at least one point in the cell, flag (1) int32 |= 1 when a point with a non-finite coordinate was left out, |= 2
 * when no cell is admissible.  cells (s,p) int32 or NULL: every point's cell (-1 for a point left out).  Integer atomics only: the
 * result does not depend on the order of points or clouds.  Returns -2 for sp < 3, r outside [2, 32], s * p > 2^31 - 1 or a NULL
 * pointer other than cells; 0 without a launch when s or p is 0. */
SLIDE_API int slide_occupancy_grid(int s, int p, const float *pts, int sp, int r, const float *axis, const uint32_t *rowmask,
                                   int *counts, int *clouds, int *cells, int *flag, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 5: DPSR, oriented points -> Poisson indicator grid */
/* The forward of the reference's pointnet2/dpsr_utils/dpsr.py (DPSR.forward) in separately callable launches; the arithmetic of
 * every step is written out in csrc/dpsr.hip.  Grids are cubic, r cells per axis, flat index (i r + j) r + k; complex arrays are
 * interleaved (re, im) floats; h = r / 2 + 1.  The FFT entry points take r in {16, 32, 64, 128, 256} (-2 otherwise); every entry
 * point returns -2 for a NULL array or an argument out of range and 0 without a launch for an empty batch.
 *
 * Trilinear scatter.  pts (b,n,3) f32 coordinates in [0, 1), vals (b,n,nf) f32, nf 1 or 3 -> grid (b,nf,r,r,r) int64, ACCUMULATED
 * into (the caller zero-fills): every point adds llrint(fl(w_c * v) * 2^32) to the 8 corners of its cell (periodic wrap of the last
 * cell) with integer atomics -- exact, independent of order and batch.  flag (1) int32 |= 1 when a point was left out: a non-finite
 * coordinate or value, a coordinate outside [0, 1), |v| >= 2^20.  2 <= r <= 1024. */
SLIDE_API int slide_point_rasterize(int b, int n, int nf, int r, const float *pts, const float *vals, long long *grid, int *flag,
                                    slide_stream_t stream);
/* out[i] = fl(fl(grid[i]) * 2^-32): the fixed-point grid as floats (what slide_fft3_r2c reads with fixed_point = 1) */
SLIDE_API int slide_grid_fixed_to_float(long long count, const long long *grid, float *out, slide_stream_t stream);
/* Trilinear gather (the reference's grid_interp).  grid (b,r,r,r,c) f32, pts (b,n,3) in [0, 1) -> out (b,n,c), the 8 corners summed
 * in corner order; same cell arithmetic and wrap as the scatter.  flag |= 1 for a coordinate outside [0, 1) (its outputs are 0). */
SLIDE_API int slide_grid_interp(int b, int n, int c, int r, const float *grid, const float *pts, float *out, int *flag,
                                slide_stream_t stream);
/* 3-D real FFT of nb grids (numpy's rfftn over the three grid axes): in (nb,r,r,r), f32 or with fixed_point != 0 the int64 grid of
 * slide_point_rasterize (read times 2^-32) -> spec (nb,r,r,h) complex.  Three launches: axis 3, then axes 2 and 1 in place. */
SLIDE_API int slide_fft3_r2c(int nb, int r, const void *in, int fixed_point, float *spec, slide_stream_t stream);
/* Its inverse (numpy's irfftn(s = (r,r,r))): spec (nb,r,r,h) complex, OVERWRITTEN (axes 1 and 2 are transformed in place) -> out
 * (nb,r,r,r) f32.  The last launch extends every axis-3 line Hermitian-symmetrically, dropping the imaginary part of bins 0 and
 * r/2, and scales by 1 / r^3. */
SLIDE_API int slide_fft3_c2r(int nb, int r, float *spec, float *out, slide_stream_t stream);
/* The spectral Poisson solve: spec (b,3,r,r,h) complex, g (r,r,h) f32 (the module's Gaussian filter) -> phis (b,r,r,h) complex,
 * sum_d(-i omega_d g spec_d) / (-|omega|^2 + 1e-6) with omega_d = fl(k_d * fl(2 pi)) and bin (0,0,0) = 0. */
SLIDE_API int slide_dpsr_spectral(int b, int r, const float *spec, const float *g, float *phis, slide_stream_t stream);
/* Shift and scale in place: offset = mean_n fv (b,n) when shift (a fixed-order sum, no atomics), else 0; phi (b,r,r,r) -= offset; then
 * with a = |phi[.,0,0,0]| read AFTER the shift, phi = -phi / a * 0.5 when scale.  coef (b,2) f32 receives (offset, a).  Two launches;
 * none when neither flag is set. */
SLIDE_API int slide_dpsr_finish(int b, int n, int r, const float *fv, int shift, int scale, float *coef, float *phi,
                                slide_stream_t stream);
/* All of it for b samples: pts / normals (b,n,3), g (r,r,h) -> phi (b,r,r,r).  Workspaces of the caller: ws_grid (b,3,r,r,r) int64
 * (zero-filled here), ws_spec (b,3,r,r,h) complex, ws_phis (b,r,r,h) complex, ws_fv (b,n) f32, ws_coef (b,2) f32; flag as above
 * (the caller zero-fills).  A sample's result does not depend on b or on its position. */
SLIDE_API int slide_dpsr_grid(int b, int n, int r, const float *pts, const float *normals, const float *g, int shift, int scale,
                              long long *ws_grid, float *ws_spec, float *ws_phis, float *ws_fv, float *ws_coef, float *phi, int *flag,
                              slide_stream_t stream);

/* The backward of slide_dpsr_grid (csrc/dpsr_bwd.hip, where the mathematics is written out): gout = dL/dphi (b,r,r,r) -> dv, dn
 * (b,n,3), the gradients of pts and normals.  phi (b,r,r,r) is the forward's output and coef (b,2) what it left in ws_coef.  No
 * atomics but the integer ones of slide_point_rasterize: every result is bit-reproducible and does not depend on b or on a
 * sample's position.
 *
 * Per-sample sums in double, fixed order: sums (b,2) = (sum gout, sum gout * phi) over a sample's r^3 cells.  ws_part (b, nbps, 2)
 * double with nbps = ceil(r^3 / 4096).  Two launches.  2 <= r <= 1024. */
SLIDE_API int slide_dpsr_bwd_sums(int b, int r, const float *gout, const float *phi, double *ws_part, double *sums,
                                  slide_stream_t stream);
/* The adjoint of slide_dpsr_finish and of the shift, elementwise: gout, phi, sums, coef and, with shift, w (b,r,r,r) int64 =
 * slide_point_rasterize(pts, 1.0) -> dpre (b,r,r,r) f32, the gradient of the grid before shift and scale.  Without shift and scale
 * it copies gout; phi, sums, coef may then be NULL, and w whenever shift is 0. */
SLIDE_API int slide_dpsr_bwd_dpre(int b, int n, int r, const float *gout, const float *phi, const double *sums, const float *coef,
                                  const long long *w, int shift, int scale, float *dpre, slide_stream_t stream);
/* The adjoint of slide_dpsr_spectral: spec (b,r,r,h) complex = slide_fft3_r2c(dpre), g (r,r,h) -> out (b,3,r,r,h) complex,
 * +i omega_d g spec / (-|omega|^2 + 1e-6), bin (0,0,0) = 0; slide_fft3_c2r of it is the gradient of the rasterized normals. */
SLIDE_API int slide_dpsr_spectral_adj(int b, int r, const float *spec, const float *g, float *out, slide_stream_t stream);
/* One thread per point: dras (b,3,r,r,r) f32 and, with shift, phi, sums and coef -> dv, dn (b,n,3); either may be NULL (0 without a
 * launch when both are).  flag as in slide_grid_interp; a point left out gets zeros. */
SLIDE_API int slide_dpsr_bwd_points(int b, int n, int r, const float *pts, const float *normals, const float *dras, const float *phi,
                                    const double *sums, const float *coef, int shift, int scale, float *dv, float *dn, int *flag,
                                    slide_stream_t stream);
/* All of it for b samples.  Workspaces of the caller: ws_w (b,r,r,r) int64 and ws_ones (b,n) f32 (both filled here; NULL allowed
 * without shift), ws_dpre (b,r,r,r) f32, ws_spec (b,r,r,h) complex, ws_spec3 (b,3,r,r,h) complex, ws_dras (b,3,r,r,r) f32, ws_part
 * and ws_sums as above (NULL allowed without shift and scale, like coef).  r in {16, 32, 64, 128, 256}, n >= 1. */
SLIDE_API int slide_dpsr_grid_bwd(int b, int n, int r, const float *pts, const float *normals, const float *g, const float *phi,
                                  const float *coef, const float *gout, int shift, int scale, long long *ws_w, float *ws_ones,
                                  float *ws_dpre, float *ws_spec, float *ws_spec3, float *ws_dras, double *ws_part, double *ws_sums,
                                  float *dv, float *dn, int *flag, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 6: marching cubes, grid -> indexed triangle mesh */
/* phi (b,r,r,r) f32, flat index (i r + j) r + k, 2 <= r <= 256 (any r, not only the FFT sizes).  A grid point is inside iff
 * phi < level (a NaN is outside).  One vertex per grid edge whose ends differ in that predicate, at p + t e_axis with
 * t = (level - a) / (b - a) in fp32 (a at the lower-index end p); its normal is the central-difference gradient of phi (one-sided on
 * the border) at the edge's two ends, interpolated with t, normalised and NEGATED (0 for a zero gradient); every cell emits the
 * triangles of its 8-bit case from csrc/marching_cubes_table.h, wound so that (v1 - v0) x (v2 - v0) points toward increasing phi.
 * The arithmetic, the brick decomposition and the order of the output are written out in csrc/marching_cubes.hip.  No atomics: a
 * grid's mesh is bit-identical in any batch, at any position and over repeated runs.  Both entry points return -2 for r outside
 * [2, 256], b < 0, a NULL pointer with b > 0 or more than 2^31 - 1 workgroups (b * slide_mc_bricks(r)), and 0 without a launch for
 * b = 0.
 *
 * The number of bricks (workgroups) per grid of size r; -2 for r outside [2, 256]. */
SLIDE_API int slide_mc_bricks(int r);
/* Count: counts_ws (b, slide_mc_bricks(r), 2) int32 receives every brick's first vertex and first triangle WITHIN its grid (the
 * exclusive prefix of the brick counts, in brick order); totals (b,4) int64 = per grid (V, F, the grid's first row in verts /
 * normals, its first row in faces) when the b meshes are stored one after the other.  Three launches.  The caller reads totals to
 * size the outputs. */
SLIDE_API int slide_mc_count(int b, int r, const float *phi, float level, int *counts_ws, long long *totals, slide_stream_t stream);
/* Emit, with counts_ws and totals as slide_mc_count left them (same phi, level): verts, normals (sum V, 3) f32, verts in grid-index
 * units; faces (sum F, 3) int32, vertex indices LOCAL to the grid (0 .. V - 1); ws (b,r,r,r) int32 workspace.  Two launches.  Not
 * to be called when sum V is 0 (there is nothing to write and the output pointers would be NULL). */
SLIDE_API int slide_mc_emit(int b, int r, const float *phi, float level, const int *counts_ws, const long long *totals, float *verts,
                            float *normals, int *faces, int *ws, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 7: area-weighted point samples from triangle meshes */
/* A batch of b meshes is PACKED, as the marching cubes above leave it: verts (sum V, 3) f32, faces (sum F, 3) int32 with vertex
 * indices LOCAL to the mesh, optional vertex normals (sum V, 3) f32, voff / foff (b + 1) int64 = every mesh's first row in verts /
 * faces, non-decreasing, voff[b] = sum V, foff[b] = sum F.  fp32 with contraction off unless it says double or integer
 * (csrc/mesh_sample.hip writes the same definition out with the launch structure):
 *
 *   n_f = (v1 - v0) x (v2 - v0), each component a*b - c*d as two products and one subtraction;
 *   area_f = 0.5f * sqrtf(n.n) with n.n = (nx*nx + ny*ny) + nz*nz;  amax = the largest finite area of the mesh;
 *   q_f = (uint64) floor((double)area_f * 2^32 / (double)amax), 0 for a zero or non-finite area or amax = 0;
 *   cdf_f = q_0 + ... + q_f within the mesh (inclusive, uint64, exact in any order);  total = cdf_{F-1} < 2^63.
 *   Faces smaller than amax 2^-32 are never drawn: the only bias.
 *
 * Sample s of mesh m takes four 32-bit words (c0, c1, c2, c3): the caller's `words`, or one Philox4x32-10 call with key
 * (seed_lo, seed_hi) and counter (s, mesh_id[m], stream_id, 0x13198A2E) (slide_philox_normal_selftest's constant is 0x85A308D3):
 *
 *   r = c0 << 32 | c1;  t = mulhi64(r, total) in [0, total);  face = the number of cdf entries <= t (a face with q = 0 is never chosen);
 *   u = ((float)(c2 >> 8) + 0.5f) * 2^-24, v likewise from c3 (the uniform of philox_normal; in (0, 1]);
 *   su = sqrtf(u), w0 = 1 - su, w1 = su * (1 - v), w2 = su * v (pytorch3d's weights);  p = (w0*v0 + w1*v1) + w2*v2;
 *   normal = n_f / max(|n_f|, FLT_EPSILON), or with vertex_normals g / max(|g|, FLT_EPSILON), g = (w0*g0 + w1*g1) + w2*g2.
 *
 * A mesh's samples depend on (mesh, seed, mesh_id, stream_id, s) alone: not on b, the mesh's position or a chunking of the batch.
 * Both entry points return -2 for a negative count or a NULL array before any launch, and 0 without a launch for b = 0 (and for
 * sum F = 0 / s = 0).
 *
 * The spans of the cdf scan, in faces: level 0 one thread, 1 one wave, 2 one pass of a mesh's workgroup; -2 otherwise. */
SLIDE_API int slide_mesh_cdf_span(int level);
/* areas (sum F) f32 and cdf (sum F) uint64, nf = sum F <= 2^31 - 1.  A face with a vertex index outside [0, V) of its mesh -- tested
 * BEFORE it is used -- sets flag |= 1, one with a non-finite coordinate flag |= 2 (flag (1) int32, zero-filled by the caller); either
 * gets area 0, hence q = 0.  Two launches: a thread per face, then one workgroup per mesh (maximum, quantise, scan). */
SLIDE_API int slide_mesh_face_cdf(int b, long long nf, const float *verts, const int *faces, const long long *voff,
                                  const long long *foff, float *areas, unsigned long long *cdf, int *flag, slide_stream_t stream);
/* s samples per mesh with cdf as slide_mesh_face_cdf left it (same arrays): points (b,s,3) f32, valid (b) int32, and when not NULL
 * normals (b,s,3) f32 and face_idx (b,s) int32 (the face's row WITHIN its mesh).  mesh_ids (b) int32 or NULL (mesh m gets m); words
 * (b,s,4) uint32, 16-byte aligned, or NULL (Philox); seed_lo, seed_hi, stream_id carry the bit patterns of unsigned words.
 * vertex_normals != 0 needs vnormals and normals.  A mesh without faces or with total = 0 gets points = normals = 0, face_idx = -1
 * and valid = 0 (else 1).  One launch, a thread per sample; b <= 65535. */
SLIDE_API int slide_mesh_sample(int b, int s, const float *verts, const int *faces, const float *vnormals, const long long *voff,
                                const long long *foff, const unsigned long long *cdf, int seed_lo, int seed_hi, int stream_id,
                                const int *mesh_ids, const unsigned *words, int vertex_normals, float *points, float *normals,
                                int *face_idx, int *valid, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 8: connected components of triangle meshes, keep-largest filter */
/* Mesh clean-up (the reference's verts_on_largest_mesh, pointnet2/dpsr_utils/utils.py: igl connected_components and trimesh split on
 * the host, one mesh at a time) for a PACKED batch as in Part 7.  Integers only; vertex coordinates play no part in labelling.
 *
 *   graph       the nodes are the mesh's V vertices; any two DISTINCT indices of one face are joined.  (a, a, b) gives the edge a-b,
 *               (a, a, a) none (it still belongs to a's component).  A vertex no face refers to is a component of its own.
 *   root[v]     the smallest vertex index of v's component: a function of the mesh alone.
 *   cid[v]      the rank of root[v] among the mesh's roots in ascending order, 0 .. C-1 (scipy's and igl's numbering).
 *   counts      nverts[c]; nfaces[c] = the faces whose FIRST index lies in c.
 *   selection   candidates are the components with nfaces >= 1 whose size (by = 0: nverts, 1: nfaces) is >= min_size.  keep_all = 0
 *               keeps the largest candidate, ties to the lowest cid (numpy argmax); keep_all != 0 keeps every candidate.  No
 *               candidate: the mesh comes out empty.
 *   compaction  kept vertices and kept faces (those whose first vertex is kept) keep their relative order and winding; vertex and
 *               normal rows are copied bit for bit; face indices are renumbered.  Every output vertex has an output face.
 *   refusal     a face index outside [0, V) of its mesh is tested BEFORE it is used as an address: the face joins nothing and
 *               info[0] = 1 (slide_mesh_cc_label); later stages skip such a face.
 *
 * Labelling: L[v] = v; a ROUND is two launches: hook (a thread per face: m = the minimum of the three labels and of THEIR labels,
 * integer atomicMin of m into the three vertices and into their labels) and jump (a thread per vertex: L[v] = L[L[..L[v]]], at most
 * 8 steps).  Labels only decrease, stay inside the component and are bounded below by its root, so a stale read within a launch is
 * an older upper bound: it can cost a round, never the result.  A round that lowers nothing was read entirely fresh, and then every
 * face has equal labels and L[L[v]] = L[v]: L is constant on a component, and since L[root] = root that constant is the root.  The
 * fixed point is unique, so the labels do not depend on the execution order, the batch or the position.
 * Cap: launches are ordered, so at a round's start every label a previous round wrote is visible.  By induction a vertex at graph
 * distance d from its root holds the root after round d (its neighbour at distance d - 1 held it at the round's start, and their
 * common face writes it); round d + 1 then changes nothing.  max_rounds = (largest V of the batch) + 1 therefore always suffices;
 * meshes from marching cubes need about log2 V rounds.  More rounds than max_rounds return -5 (never an unbounded loop).
 * The host reads two words (refusal, last round that lowered a label) once per `group` rounds and synchronises the stream for it:
 * slide_mesh_cc_label is the one entry point here that BLOCKS.  Surplus rounds at the fixed point change nothing.
 * No float atomics, no spin-waiting, no inter-workgroup barrier: every launch is one grid over the packed faces or vertices.
 *
 * Limits: sum V and sum F <= 2^31 - 1, b <= 65535.  All four entry points return -2 for a count out of range or a NULL array before
 * any launch and 0 without a launch for b = 0 or sum V = 0.
 *
 * Spans, in elements: level 0 one workgroup of the per-face / per-vertex launches, 1 one wave of a scan, 2 one pass of a mesh's
 * workgroup in a scan; -2 otherwise. */
SLIDE_API int slide_mesh_cc_span(int level);
/* labels (sum V) int32 receives root[v] (LOCAL index).  state (2) int32 is device scratch.  info (4) int32 on the HOST receives
 * {refusal flag, rounds that lowered a label, host reads, rounds issued}.  group >= 1 rounds per host read, max_rounds >= 1. */
SLIDE_API int slide_mesh_cc_label(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff,
                                  int *labels, int *state, int group, int max_rounds, int *info, slide_stream_t stream);
/* With labels as slide_mesh_cc_label left them: cnt_v, cnt_f (sum V) int32 = vertices / faces per component AT ITS ROOT's row (int32
 * atomic adds: exact, order-free), rank (sum V) int32 = the cid at every root's row (other rows are not written), cid (sum V) int32,
 * nverts / nfaces (sum V) int32 whose first C rows of every mesh (from voff[m]) hold the counts by cid, totals (b, 4) int32 whose
 * column 2 receives C.  Two memsets and two launches: counts, then one workgroup per mesh (scan of the root flags in passes). */
SLIDE_API int slide_mesh_cc_stats(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff,
                                  const int *labels, int *cnt_v, int *cnt_f, int *rank, int *cid, int *nverts, int *nfaces, int *totals,
                                  slide_stream_t stream);
/* Selection and the two exclusive scans, one workgroup per mesh: vnew (sum V) / fnew (sum F) int32 = the row's place among the kept
 * rows of its mesh, or -1; totals columns 0, 1, 3 receive V', F' and the selected root (-1: none, or keep_all). */
SLIDE_API int slide_mesh_cc_select(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff,
                                   const int *labels, const int *cnt_v, const int *cnt_f, int by, long long min_size, int keep_all,
                                   int *vnew, int *fnew, int *totals, slide_stream_t stream);
/* One launch over the packed vertices and faces: out_verts (sum V', 3), out_normals (or NULL with normals NULL), vert_idx (sum V')
 * int32 = the row's index in its input mesh, out_faces (sum F', 3) int32.  ovoff / ofoff (b + 1) int64: the prefix sums of V' / F'. */
SLIDE_API int slide_mesh_cc_compact(int b, long long nv, long long nf, const float *verts, const float *normals, const int *faces,
                                    const long long *voff, const long long *foff, const int *vnew, const int *fnew,
                                    const long long *ovoff, const long long *ofoff, float *out_verts, float *out_normals,
                                    int *out_faces, int *vert_idx, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 9: refine-and-upsample front of DPSR */
/* What the reference does around its refinement network before DPSR sees a cloud (pointnet2/data_utils/mirror_partial.py,
 * models/point_upsample_module.py, the tail of network_output_to_dpsr_grid in dpsr_evaluation.py).  All arithmetic is fp32, every
 * product, sum and quotient rounded once in the order written (the file is compiled with contraction off; `/` is the correctly
 * rounded division), so the outputs equal the reference's bit for bit.  No float atomics; no launch reads what another workgroup of
 * the same launch wrote; the results of a sample do not depend on the batch, its position or the run.
 *
 * Both entry points own a flag (2) int32 on the device: they reset it themselves, flag[0] collects the bits named below and flag[1]
 * the largest (sample + 1) that set one.  The caller reads it once.
 * Status: -2 a negative count, b > 65535, a NULL array or a misaligned disp; -3 ldx not 6 or 7; -4 a disp width dw that does not match
 * the form; -5 include_center without first_refine; -6 factor < 1.  0 without a launch for an empty batch.
 *
 * slide_mirror_concat: x (b, n, c) f32, c >= 3, axis in {0, 1, 2}.
 *   center[s, k] = (float)(sum_i (double)x[s, i, k] / (double)n), the sum in a fixed order (a thread's rows ascending, then a tree
 *                  over the workgroup's threads);  center (b, 3) is an output.
 *   mirrored row  for k < 3:  m = x[k] - center[k];  m = -m on k == axis;  m = m + center[k]  (the centre is added back on the two
 *                 untouched axes too, as the reference does: that can move them by an ulp).  Channel axis + 3 is negated when
 *                 c >= 6; other channels are copied.
 *   out (b, 2n, c + attach_label): row j is row perm[j] (or j with perm NULL) of [the n original rows, label +1; the n mirrored rows,
 *                 label -1].  perm (2n) int32 is shared by the batch.  An entry outside [0, 2n) is tested BEFORE it is used: the row
 *                 is filled with zeros and flag[0] |= 1.
 *   Two launches: the centres (one workgroup per sample), then a thread per output row. */
SLIDE_API int slide_mirror_concat(int b, int n, int c, const float *x, int axis, int attach_label, const int *perm, float *out,
                                  float *center, int *flag, slide_stream_t stream);
/* slide_refine_to_dpsr: X (b, m, ldx) f32 whose first 6 channels are xyz + normal (ldx 7: an indicator behind them, not read), disp
 * (b, m, dw) f32, 8-byte aligned; the first `rows` <= m rows of every sample are split (only_original_points_split: rows = m / 2).
 *   g = (float)(1 / sqrt((double)factor)), s = out_scale, kp = children per point, R = output rows per sample:
 *   plain form                       dw = 6 factor        kp = factor      child[n, j, c] = X[n, c] + (disp[n, 6 j + c] * g) * s
 *   first_refine                     dw = 6 (factor + 1)  kp = factor      mid[n, c] = X[n, c] + disp[n, c] * s
 *                                                                          child[n, j, c] = mid[n, c] + (disp[n, 6 + 6 j + c] * g) * s
 *   first_refine and include_center  dw = 6 factor        kp = factor - 1  as above, and the rows mid[n] follow all the children
 *   Child (n, j) is output row n kp + j; R = rows kp (+ rows).  c = 0..2 are the position, 3..5 the normal (not renormalised).
 *   bbox[s] = {mn, mx}: the minimum and maximum over the sample's R output positions, per axis (a NaN takes no part).
 *   mode 0 (normalize)  ctr = (mx + mn) / 2;  L = max over the axes of (mx - mn);  p = (child - ctr) / L * 0.99f
 *   mode 1 (scale)      p = child / scale / 2
 *   points = min(max(p / 1.2f + 0.5f, 0), 0.99f);  normals = the child's channels 3..5.
 *   flag[0] |= 1 for a non-finite child position (tested explicitly: fminf drops a NaN), |= 2 for L == 0 in mode 0.
 *   Outputs: points, normals (b, R, 3), bbox (b, 2, 3).  partials (b, T, 6) f32 is scratch, T = ceil(R / slide_refine_span(0)).
 *   Two launches over (tile, sample): every workgroup stores the minimum and maximum of its tile of slide_refine_span(0) rows (a wave
 *   reduction, then LDS; plain stores); then every workgroup reduces its sample's partials and transforms its tile.  A thread owns one
 *   output row and reads its six displacements as three 8-byte words. */
SLIDE_API int slide_refine_span(int level); /* level 0: the output rows of one tile; -2 otherwise */
SLIDE_API int slide_refine_to_dpsr(int b, int m, int ldx, int dw, int rows, const float *X, const float *disp, int factor, int first_refine,
                                   int include_center, float out_scale, int mode, float scale, float *points, float *normals,
                                   float *bbox, float *partials, int *flag, slide_stream_t stream);

/* ------------------------------------------------------------------ Part 3: denoiser engine */
/* see slide_engine.h */
SLIDE_API const char *slide_hip_version(void);
SLIDE_API int slide_hip_device_ok(void); /* 1 if a gfx950 device is visible */

/* Self-test of the GroupNorm epilogues' lane reduction (csrc/lane_reduce.h): ONE 64-lane wave sums nv (4, 8, 16, 32 or 64) fp32
 * values per lane over each 32-lane half wave, twice.  in (64,nv): lane l's values.  out_old (64,nv): the all-reduce
 * lane_group_sum<32> of every value, as every lane holds it.  out_new (64, max(nv / 32, 1)): what lane_half_sums leaves in the
 * lane's registers; register j is the total of value lane_reduce_index<nv>(l) + j (the rule is written out in lane_reduce.h).
 * Returns -2 for another nv or a NULL pointer. */
SLIDE_API int slide_lane_reduce_selftest(const float *in, float *out_new, float *out_old, int nv, slide_stream_t stream);

/* Self-test of the noise the DDPM update kernels draw in registers (csrc/ddpm_update.h philox_normal: Philox4x32-10 keyed with the
 * seed on the counter (element, step, 0x243F6A88 ^ nonce, 0x85A308D3), Box-Muller on the first two output words):
 * out[i] = philox_normal(seed, step, elem0 + i, nonce) for i < n (element numbers wrap at 2^32).  seed_lo .. elem0 carry the bit
 * patterns of 32-bit unsigned words.  Returns -2 for n < 0 or a NULL out with n > 0; n == 0 launches nothing. */
SLIDE_API int slide_philox_normal_selftest(int seed_lo, int seed_hi, int step, int nonce, int elem0, int n, float *out,
                                           slide_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
