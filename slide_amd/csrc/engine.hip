// engine.hip -- the op dispatcher and the runtime API of the fused latent-DDPM denoiser for gfx950 (C-ABI:
// include/slide_engine.h), with the small per-step kernels (prep / assemble / finalize / t-embedding / condition / DDPM update /
// transpose / NCHW GroupNorm).  The GEMM kernels are in gemm_ring.hip, gemm_gx.hip, gemm_gxs.hip and sa_chain.hip, the
// pair-table pass in pair_norm.hip, the fused attention tails in attn_tail.hip and attn_tail_split.hip; what crosses translation
// units is declared in launch.h, which is also the map of which file defines what.
#include "gemm_common.h"
#include "ddpm_update.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

// ------------------------------------------------------------------------------------------------ points
// Per sample (16 latent points): split x into xyz + features [x[3:], xyz] (attach_position_to_input_feature,
// pointnet2_with_pcld_condition.py:332-346) and build the full 16x16 neighbour table sorted by
// (squared distance, index) -- the K=16 and K=8 queries of every SA / FP level are prefixes of it
// (knn_points semantics, oracle/ops_cpu.c ora_knn_points).
template <typename T>
__global__ __launch_bounds__(256) void prep_points_kernel(int cx, int ldf, const float *__restrict__ x,
                                                          float *__restrict__ xyz, T *__restrict__ feat0,
                                                          int *__restrict__ kidx, float *__restrict__ kd2,
                                                          T *__restrict__ feat0_cm, const SlidePrepCopy *__restrict__ copies,
                                                          int n_copies, float *__restrict__ kw) {
  __shared__ float sp[48];
  __shared__ float sd[16][17];
  __shared__ float ssort[16][17];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float *xb = x + (size_t)b * 16 * cx;
  if (tid < 48) {
    const float v = xb[(tid / 3) * cx + tid % 3];
    sp[tid] = v;
    xyz[(size_t)b * 48 + tid] = v;
  }
  const int nf = cx - 3;
  for (int e = tid; e < 16 * cx; e += 256) {
    const int p = e / cx, c = e % cx;
    const T v = (T)(c < nf ? xb[p * cx + 3 + c] : xb[p * cx + (c - nf)]);
    feat0[((size_t)b * 16 + p) * ldf + c] = v;
    // second, chunk-major copy [c / 32][samples * 16][32] for the gather-on-load GEMM of the first SA block
    if (feat0_cm) feat0_cm[((size_t)(c >> 5) * gridDim.x * 16 + (size_t)b * 16 + p) * 32 + (c & 31)] = v;
  }
  // columns of later concatenation buffers that hold nothing but this sample's features / coordinates (the skip input and
  // the xyz columns of the FP blocks' second Mlp, the xyz columns of the head): written here instead of by COPY launches
  for (int q = 0; q < n_copies; ++q) {
    const SlidePrepCopy cp = copies[q];
    T *dst = reinterpret_cast<T *>(cp.dst);
    for (int e = tid; e < 16 * cp.n; e += 256) {
      const int p = e / cp.n, c = e - p * cp.n;
      const float v = cp.kind ? xb[p * cx + c] : (c < nf ? xb[p * cx + 3 + c] : xb[p * cx + (c - nf)]);
      dst[((size_t)b * 16 + p) * cp.ld + c] = (T)v;
    }
  }
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  const float d = sqdist3(sp[i * 3], sp[i * 3 + 1], sp[i * 3 + 2], sp[j * 3], sp[j * 3 + 1], sp[j * 3 + 2]);
  sd[i][j] = d;
  __syncthreads();
  int rank = 0;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const float o = sd[i][jj];
    rank += (o < d || (o == d && jj < j)) ? 1 : 0;
  }
  kidx[((size_t)b * 16 + i) * 16 + rank] = j;
  kd2[((size_t)b * 16 + i) * 16 + rank] = d;
  if (kw) {  // group_knn's interpolation weights of the 8 nearest, from SQUARED distances (pointnet2_utils.py:510-513)
#pragma clang fp contract(off)
    ssort[i][rank] = d;
    __syncthreads();
    float norm = 0.f;
    for (int kk = 0; kk < 8; ++kk) norm += 1.0f / (ssort[i][kk] + 1e-8f);
    kw[((size_t)b * 16 + i) * 16 + j] = j < 8 ? (1.0f / (ssort[i][j] + 1e-8f)) / norm : 0.f;
  }
}

// QueryAndGroup feature assembly ('nn', use_xyz, abs + center coordinates; pointnet2_utils.py:383-430):
// g[b][p*K+k][:] = [feat[nbr][0:C], xyz[nbr]-xyz[p], xyz[nbr], xyz[p], 0-pad]
// group_knn feature assembly (pointnet2_utils.py:497-524), FP = true:
// g[b][p*K+k][:] = [feat[nbr][0:C], d2, w, xyz[nbr], xyz[nbr]-xyz[p], xyz[p], 0-pad], w from squared distances
// One thread moves 8 channels (16 bytes in fp16): the gathered feature rows are copied as whole vectors, only the
// chunk that holds the coordinate channels is assembled element-wise.
template <typename T, bool FP>
__global__ __launch_bounds__(256) void assemble_kernel(int C, int ldf, int ldg, int K, int nch_log2, int bulk_blocks,
                                                       int c_begin, int ld_out,
                                                       const float *__restrict__ xyz,
                                                       const T *__restrict__ feat, const int *__restrict__ kidx,
                                                       const float *__restrict__ kd2, T *__restrict__ g) {
#pragma clang fp contract(off)
  // one thread per (row, 16-byte piece), no integer division.  Blocks y < bulk_blocks copy the whole-vector pieces of
  // the gathered feature rows (piece = low `nch_log2` bits of the thread id); the remaining blocks assemble the pieces
  // that hold coordinate channels element-wise -- kept in separate waves so the copy waves never diverge into that path.
  const int b = blockIdx.x;
  const int npx = 16 * K;
  const int nch = ldg / 8;
  const int nbulk = (sizeof(T) * ldf % 16 == 0) ? C / 8 : 0, ntail = nch - nbulk;
  const float *px = xyz + (size_t)b * 48;
  {
    int pxl, c0;
    if ((int)blockIdx.y < bulk_blocks) {
      const int e = blockIdx.y * 256 + threadIdx.x;
      pxl = e >> nch_log2;
      c0 = c_begin + (e & ((1 << nch_log2) - 1)) * 8;  // c_begin > 0: the leading columns are gathered by the GEMM itself
      if (pxl >= npx || c0 >= nbulk * 8) return;
    } else {
      const int e = (blockIdx.y - bulk_blocks) * 256 + threadIdx.x;
      pxl = e / ntail;
      c0 = (nbulk + (e - pxl * ntail)) * 8;
      if (pxl >= npx) return;
    }
    const int p = pxl / K, k = pxl - p * K;
    const size_t o = ((size_t)b * 16 + p) * 16;
    const int nb = kidx[o + k];
    const T *frow = feat + ((size_t)b * 16 + nb) * ldf;
    T *dst = g + ((size_t)b * npx + pxl) * ld_out + (c0 - c_begin);
    if (c0 + 8 <= C && sizeof(T) * ldf % 16 == 0) {
      if (sizeof(T) == 2) {
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(frow + c0);
      } else {
        *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(frow + c0);
        *reinterpret_cast<float4 *>(dst + 4) = *reinterpret_cast<const float4 *>(frow + c0 + 4);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      float v = 0.f;
      if (c < C) v = (float)frow[c];
      else if (!FP) {
        if (c < C + 3) v = px[nb * 3 + (c - C)] - px[p * 3 + (c - C)];
        else if (c < C + 6) v = px[nb * 3 + (c - C - 3)];
        else if (c < C + 9) v = px[p * 3 + (c - C - 6)];
      } else {
        if (c == C) v = kd2[o + k];
        else if (c == C + 1) {
          float norm = 0.f;
          for (int kk = 0; kk < K; ++kk) norm += 1.0f / (kd2[o + kk] + 1e-8f);
          v = (1.0f / (kd2[o + k] + 1e-8f)) / norm;
        } else if (c < C + 5) v = px[nb * 3 + (c - C - 2)];
        else if (c < C + 8) v = px[nb * 3 + (c - C - 5)] - px[p * 3 + (c - C - 5)];
        else if (c < C + 11) v = px[p * 3 + (c - C - 8)];
      }
      dst[j] = (T)v;
    }
  }
}

// GroupNorm over a channel-concatenated tensor whose groups straddle producers (attention weight_conv.1,
// attention.py:45-47): per-sample channel sums -> per-channel scale / shift applied by the consumer GEMM.
__global__ __launch_bounds__(256) void finalize_gn_kernel(int B, int C, int bs, float inv_count,
                                                          const float *__restrict__ sum, const float *__restrict__ sq,
                                                          const int *__restrict__ gid, const int *__restrict__ gstart,
                                                          const int *__restrict__ gend, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float *__restrict__ scale,
                                                          float *__restrict__ shift) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * C) return;
  const int b = e / C, c = e - b * C;
  const int g = gid[c];
  float sc = 1.f, sh = 0.f;
  if (g >= 0) {
    // no FMA contraction: the small-launch GEMM that finalises the statistics itself (gemm_small.h) must round the same
    // operations the same way -- a one-ulp difference of a scale flips its fp16 rounding in a few samples
#pragma clang fp contract(off)
    float S = 0.f, SS = 0.f;
    for (int cc = gstart[g]; cc < gend[g]; ++cc) {
      S += sum[(size_t)b * bs + cc];
      SS += sq[(size_t)b * bs + cc];
    }
    const float mean = S * inv_count;
    const float var = fmaxf(SS * inv_count - mean * mean, 0.f);
    const float rstd = 1.0f / sqrtf(var + GN_EPS);
    sc = gamma[c] * rstd;
    sh = beta[c] - mean * sc;
  }
  scale[(size_t)b * bs + c] = sc;
  shift[(size_t)b * bs + c] = sh;
}

// out[bp][c] = sum_k softmax_k(S[bp*K+k][c]) * V[bp*K+k][c]     (attention.py:90-95, mask == all ones)
template <int K, typename T>
__global__ __launch_bounds__(256) void attn_combine_kernel(int nbp, int C, int ldS, int ldV, int ldo,
                                                           const T *__restrict__ S, const T *__restrict__ V,
                                                           T *__restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nbp * C) return;
  const int bp = e / C, c = e - bp * C;
  float s[K];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = (float)S[((size_t)bp * K + k) * ldS + c];
    m = fmaxf(m, s[k]);
  }
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = expf(s[k] - m);
    den += s[k];
  }
  float o = 0.f;
  const float inv = 1.0f / den;
#pragma unroll
  for (int k = 0; k < K; ++k) o += (float)V[((size_t)bp * K + k) * ldV + c] * (s[k] * inv);
  out[(size_t)bp * ldo + c] = (T)o;
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void copy_cols_kernel(int rows, int n, int src_ld, int dst_ld,
                                                        const TS *__restrict__ src, TD *__restrict__ dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * n) return;
  const int r = e / n, c = e - r * n;
  dst[(size_t)r * dst_ld + c] = (TD)(float)src[(size_t)r * src_ld + c];
}

// Generic GroupNorm for the module-level compatibility path: x is NCHW (B, C, HW) fp32 like the reference's tensors;
// the first n_norm channels are normalised in G groups (MyGroupNorm, pointnet2_modules.py:24-42), the rest copied.
// One workgroup per (sample, group): a group's channels are one contiguous run of gs*HW floats.
__global__ __launch_bounds__(256) void group_norm_nchw_kernel(int C, int HW, int G, int n_norm, int relu,
                                                              const float *__restrict__ x, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float *__restrict__ y) {
  __shared__ float red[2][4];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const int gs = n_norm / G;
  const size_t base = ((size_t)b * C + (size_t)g * gs) * HW;
  const int n = gs * HW;
  if (g == G) {  // pass-through tail channels
    const size_t tb = ((size_t)b * C + n_norm) * HW;
    for (int i = tid; i < (C - n_norm) * HW; i += 256) y[tb + i] = relu ? fmaxf(x[tb + i], 0.f) : x[tb + i];
    return;
  }
  float s = 0.f, ss = 0.f;
  for (int i = tid; i < n; i += 256) {
    const float v = x[base + i];
    s += v; ss += v * v;
  }
  for (int off = 32; off >= 1; off >>= 1) { s += __shfl_xor(s, off); ss += __shfl_xor(ss, off); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = ss; }
  __syncthreads();
  s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  ss = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  const float mean = s / n;
  const float var = fmaxf(ss / n - mean * mean, 0.f);
  const float rstd = 1.0f / sqrtf(var + GN_EPS);
  for (int i = tid; i < n; i += 256) {
    const int c = g * gs + i / HW;
    float v = (x[base + i] - mean) * rstd * gamma[c] + beta[c];
    y[base + i] = relu ? fmaxf(v, 0.f) : v;
  }
}

__device__ __forceinline__ float swishf(float x) { return x * (1.0f / (1.0f + expf(-x))); }

// t-embedding path (pointnet2_ssg_sem.py:14-31 + pointnet2_with_pcld_condition.py:354-359) followed by every
// Mlp_plus_t_emb.fc (pointnet2_modules.py:139-143), one workgroup per distinct timestep.
// Weights are stored input-major ([in][out]) so lanes read consecutive outputs.
__global__ __launch_bounds__(256) void temb_kernel(int t_dim, int n_out, const float *__restrict__ ts,
                                                   const int *__restrict__ t_dev, const float *__restrict__ freq,
                                                   const float *__restrict__ w1, const float *__restrict__ b1,
                                                   const float *__restrict__ w2, const float *__restrict__ b2,
                                                   const float *__restrict__ wfc, const float *__restrict__ bfc,
                                                   float *__restrict__ out) {
  extern __shared__ float sm[];
  float *emb = sm;               // t_dim
  float *h1 = sm + t_dim;        // 4*t_dim
  float *h2 = h1 + 4 * t_dim;    // 4*t_dim
  const int b = blockIdx.x, tid = threadIdx.x;
  const float t = ts ? ts[b] : (float)t_dev[0];
  const int hd = t_dim / 2, H = 4 * t_dim;
  for (int k = tid; k < hd; k += 256) {
    const float arg = t * freq[k];
    emb[k] = sinf(arg);
    emb[hd + k] = cosf(arg);
  }
  __syncthreads();
  // input-major weights: lanes read consecutive outputs; 8 loads in flight per thread (the dims are multiples of 8)
  auto gemv = [&](const float *__restrict__ in, int n_in, const float *__restrict__ w, int n_o, int j) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < n_in; k += 8) {
      const float w0 = w[(size_t)(k + 0) * n_o + j], w1_ = w[(size_t)(k + 1) * n_o + j], w2_ = w[(size_t)(k + 2) * n_o + j],
                  w3 = w[(size_t)(k + 3) * n_o + j], w4 = w[(size_t)(k + 4) * n_o + j], w5 = w[(size_t)(k + 5) * n_o + j],
                  w6 = w[(size_t)(k + 6) * n_o + j], w7 = w[(size_t)(k + 7) * n_o + j];
      a0 += in[k] * w0; a1 += in[k + 1] * w1_; a2 += in[k + 2] * w2_; a3 += in[k + 3] * w3;
      a0 += in[k + 4] * w4; a1 += in[k + 5] * w5; a2 += in[k + 6] * w6; a3 += in[k + 7] * w7;
    }
    return (a0 + a1) + (a2 + a3);
  };
  for (int j = tid; j < H; j += 256) h1[j] = swishf(b1[j] + gemv(emb, t_dim, w1, H, j));
  __syncthreads();
  for (int j = tid; j < H; j += 256) h2[j] = swishf(b2[j] + gemv(h1, H, w2, H, j));
  __syncthreads();
  for (int j = tid; j < n_out; j += 256) out[(size_t)b * n_out + j] = bfc[j] + gemv(h2, H, wfc, n_out, j);
}

// class embedding lookup (pointnet2_with_pcld_condition.py:363-365) + every Mlp_plus_t_emb.fc_condition
__global__ __launch_bounds__(256) void cond_kernel(int dim, int n_out, const int64_t *__restrict__ label,
                                                   const float *__restrict__ class_emb, const float *__restrict__ wfc,
                                                   const float *__restrict__ bfc, float *__restrict__ out) {
  extern __shared__ float sm[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float *ce = class_emb + (size_t)label[b] * dim;
  for (int k = tid; k < dim; k += 256) sm[k] = ce[k];
  __syncthreads();
  for (int j = tid; j < n_out; j += 256) {
    float acc = bfc[j];
    for (int k = 0; k < dim; ++k) acc += sm[k] * wfc[(size_t)k * n_out + j];
    out[(size_t)b * n_out + j] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ DDPM updates
// (Philox noise, timestep advance, update_feat_element: ddpm_update.h)
// Both kernels hand the timestep over with the ticket form of ddpm_update.h and are laid out around ONE exposed round trip, the read
// of t_dev: the state, the prediction and the condition do not depend on t and are requested with it; the coefficients (scalar
// loads indexed by t) are requested behind the barrier and arrive under the Philox / Box-Muller draw, which needs only step, the
// nonce and the element number.  The arithmetic, operation by operation, is update_feat_element's (ddpm_update.h).
// sampling() update (pointnet2/util.py:247-253): x = (x - c_eps[t]*eps)/sqrt_alpha[t]; t>0: x += sigma[t]*z
__global__ __launch_bounds__(256) void update_pos_kernel(int n, int eps_ld, uint32_t seed_lo, uint32_t seed_hi, float *__restrict__ x,
                                                         const float *__restrict__ eps, const float *__restrict__ noise,
                                                         int *__restrict__ t_dev, const float *__restrict__ c_eps,
                                                         const float *__restrict__ sqrt_alpha,
                                                         const float *__restrict__ sigma) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool live = e < n;
  // ---- every load that does not need t
  const int t = t_dev[0], step = t_dev[1];
  const uint32_t nonce = (uint32_t)t_dev[3], eoff = (uint32_t)t_dev[4] * 48u;
  float xv = 0.f, ev = 0.f;
  if (live) {
    xv = x[e];
    ev = eps[eps_ld ? (e / 3) * eps_ld + e % 3 : e];  // eps rows may be padded (the plan's last GEMM output)
  }
  arrived(xv);
  arrived(ev);
  t_hold(t, step);
  __syncthreads();
  int ticket = 0;
  if (threadIdx.x == 0) ticket = t_ticket_draw(t_dev);
  // ---- the coefficients (in flight under the draw)
  const float ce = c_eps[t], sa = sqrt_alpha[t], sg = sigma[t];
  float z = 0.f;
  if (t > 0 && live) {
    if (noise) {
      z = noise[(size_t)step * n + e];
      arrived(z);  // (waited for HERE, so that the path that draws its noise has no wait on loads behind the ticket)
    } else {
      z = philox_normal(seed_lo, seed_hi, (uint32_t)step, (uint32_t)e + eoff, nonce);
    }
  }
  if (live) {
    float v = (xv - ce * ev) / sa;
    if (t > 0) v = v + sg * z;
    x[e] = v;
  }
  if (threadIdx.x == 0) t_ticket_settle(t_dev, ticket, (int)gridDim.x, t, step);
}

// denoising_step (pointnet2/diffusion_utils/diffusion.py:58-95) with the key-point channels re-clamped to the
// condition (:383-385): x0 = rc*x - rm1*eps [clamp]; mean = c1*x0 + c2*x; x = mean + [t>0] std*z
//
// A thread is a (point, channel slot): lane l of a wave owns channel blockIdx.y * 64 + l of the wave's EPT consecutive points, so
// no element pays a division by C and a wave's loads and stores of a point are one contiguous run.  The first
// UPDATE_STAGED_COPIES SlidePrepCopy descriptors are read ONCE per workgroup, one per lane and together with the other first loads,
// and cross to the other lanes through LDS behind the barrier the ticket needs anyway (a plan has about six, one of them of kind 0);
// descriptors beyond those are read from memory per use.
#ifndef SLIDE_UPDATE_FEAT_EPT
#define SLIDE_UPDATE_FEAT_EPT 2  // points per wave (profiles/update_kernels.md)
#endif
constexpr int UPDATE_STAGED_COPIES = 8;

__device__ __forceinline__ void update_feat_store(void *dst, size_t i, int half_out, float v) {
  if (half_out) gptr<_Float16>((uint64_t)dst)[i] = (_Float16)v;  // (known GLOBAL: no flat stores through a loaded pointer)
  else gptr<float>((uint64_t)dst)[i] = v;
}

template <int EPT>
__global__ __launch_bounds__(256) void update_feat_kernel(int npts, int C, int kdim, int eps_ld, float clamp, uint32_t seed_lo,
                                                          uint32_t seed_hi, float *__restrict__ x,
                                                          const float *__restrict__ eps, const float *__restrict__ noise,
                                                          int *__restrict__ t_dev, const float *__restrict__ keypoint,
                                                          const float *__restrict__ rc, const float *__restrict__ rm1,
                                                          const float *__restrict__ c1, const float *__restrict__ c2,
                                                          const float *__restrict__ stdv,
                                                          const float *__restrict__ complete_x0,
                                                          const float *__restrict__ kmask, void *__restrict__ feat0, int ldf,
                                                          int half_out, const SlidePrepCopy *__restrict__ copies, int n_copies) {
#pragma clang fp contract(off)
  __shared__ u32x4 cps[UPDATE_STAGED_COPIES];
  const int tid = threadIdx.x, c = blockIdx.y * 64 + (tid & 63);
  const int p0 = (blockIdx.x * 4 + (tid >> 6)) * EPT;
  if (!feat0) n_copies = 0;
  // the integer arguments are fetched in ONE batch ahead of the t_dev read: a wait for a scalar load is a wait for all of them, so
  // an argument fetched later, where it is first used, would put the t_dev round trip in front of the loads that follow it.
  // (Not volatile and no memory clobber: either would turn the t_dev read into a vector load.  The pointers stay out: a pointer
  // that escapes into an asm statement loses its no-alias guarantee, and the coefficient reads would become vector loads.)
  asm("" : "+s"(npts), "+s"(C), "+s"(kdim), "+s"(eps_ld), "+s"(clamp), "+s"(seed_lo), "+s"(seed_hi), "+s"(ldf), "+s"(half_out),
      "+s"(n_copies));
  // ---- every load that does not need t
  const int t = t_dev[0], step = t_dev[1];
  const uint32_t nonce = (uint32_t)t_dev[3];
  // the noise element index is GLOBAL: t_dev[4] = global index of the chain's first sample, so that a shape's noise does not
  // depend on how the run was split into ranks, batches and sub-batch chains
  const uint32_t eoff = (uint32_t)t_dev[4] * (uint32_t)(16 * C);
  asm volatile("" ::: "memory");  // (the t_dev read goes out FIRST: no load below may be issued ahead of it)
  // lane q of the first wave: descriptor q (an absent one re-reads the last).  Nothing else is assigned to my_cp and nothing is
  // computed from it before the LDS write below: either puts a wait for this load in front of the element loads
  const bool stager = tid < (n_copies > 0 ? UPDATE_STAGED_COPIES : 0);
  SlidePrepCopy my_cp;
  if (stager) my_cp = copies[min(tid, n_copies - 1)];
  asm volatile("" ::: "memory");
  float xv[EPT], ev[EPT], cx0[EPT], km[EPT];
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int p = p0 + j, e = p * C + c;
    xv[j] = ev[j] = cx0[j] = km[j] = 0.f;
    if (p < npts && c < C) {
      if (c < kdim) {
        xv[j] = keypoint[(size_t)p * kdim + c];
      } else {
        xv[j] = x[e];
        if (eps) ev[j] = eps[eps_ld ? (size_t)p * eps_ld + c : (size_t)e];
        if (complete_x0) {
          km[j] = kmask[p];
          cx0[j] = complete_x0[e];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    arrived(xv[j]);
    arrived(ev[j]);
    arrived(cx0[j]);
    arrived(km[j]);
  }
  // staged as (dst, ld, n) with n = 0 for an entry that is absent or no feature copy (kind != 0).  The descriptor is opaque up to
  // here, so that nothing computed from it (and no wait for it) is placed among the loads above
  if (stager) {
    asm volatile("" : "+v"(my_cp.dst), "+v"(my_cp.ld), "+v"(my_cp.kind), "+v"(my_cp.n)::"memory");
    cps[tid] = u32x4{(uint32_t)(uint64_t)my_cp.dst, (uint32_t)((uint64_t)my_cp.dst >> 32), (uint32_t)my_cp.ld,
                     tid < n_copies && my_cp.kind == 0 ? (uint32_t)max(my_cp.n, 0) : 0u};
  } else if (tid < UPDATE_STAGED_COPIES) {
    cps[tid] = u32x4{0u, 0u, 0u, 0u};
  }
  t_hold(t, step);
  __syncthreads();  // (every wave of the workgroup holds t and step; cps is staged)
  int ticket = 0;
  if (tid == 0) ticket = t_ticket_draw(t_dev);
  u32x4 cp[UPDATE_STAGED_COPIES];
#pragma unroll
  for (int q = 0; q < UPDATE_STAGED_COPIES; ++q) cp[q] = cps[q];
  // ---- the coefficients (in flight under the draw)
  const float k_rc = rc[t], k_rm1 = rm1[t], k_c1 = c1[t], k_c2 = c2[t], k_std = stdv[t];
  float z[EPT];
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int p = p0 + j, e = p * C + c;
    z[j] = 0.f;
    if (t > 0 && p < npts && c >= kdim && c < C) {
      if (noise) {
        z[j] = noise[(size_t)step * npts * C + e];
        arrived(z[j]);  // (waited for HERE, so that the path that draws its noise has no wait on loads behind the ticket)
      } else {
        z[j] = philox_normal(seed_lo, seed_hi, (uint32_t)step, (uint32_t)e + eoff, nonce);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const int p = p0 + j, e = p * C + c;
    if (p >= npts || c >= C) continue;
    if (c < kdim) {
      x[e] = xv[j];
      continue;
    }
    float x0 = k_rc * xv[j] - k_rm1 * ev[j];
    if (clamp > 0.f) x0 = fminf(fmaxf(x0, -clamp), clamp);
    if (complete_x0)  // local re-sampling (diffusion.py:76-79): pred_xstart*mask + complete_x0*(1-mask), mask per point
      x0 = x0 * km[j] + cx0[j] * (1.f - km[j]);
    float v = k_c1 * x0 + k_c2 * xv[j];
    if (t > 0) v = v + k_std * z[j];
    x[e] = v;
    // fixed key points (kdim == 3): the feature column of the per-point table and of the concatenation buffers that the NEXT
    // step's point preparation would derive from this element (update_feat_element)
    if (feat0) {
      const int cf = c - kdim;
      update_feat_store(feat0, (size_t)p * ldf + cf, half_out, v);
#pragma unroll
      for (int q = 0; q < UPDATE_STAGED_COPIES; ++q)
        if (cf < (int)cp[q][3])
          update_feat_store((void *)((uint64_t)cp[q][1] << 32 | cp[q][0]), (size_t)p * (int)cp[q][2] + cf, half_out, v);
      for (int q = UPDATE_STAGED_COPIES; q < n_copies; ++q) {
        const SlidePrepCopy cp = copies[q];
        if (cp.kind == 0 && cf < cp.n) update_feat_store(cp.dst, (size_t)p * cp.ld + cf, half_out, v);
      }
    }
  }
  if (tid == 0) t_ticket_settle(t_dev, ticket, (int)(gridDim.x * gridDim.y), t, step);
}

// ------------------------------------------------------------------------------------------------ output head + DDPM update
// fc_lyaer (conv -> GroupNorm(32, 128) -> ReLU -> conv, pointnet2_with_pcld_condition.py:480-483) and the DDPM update of the
// sampler as ONE launch (SLIDE_OP_HEAD_UPDATE) instead of two small GEMM launches + the update kernel.  A workgroup owns 64
// rows (four samples); both layers' weights are tiny (<= 40 KB + 16 KB), so each wave loads the rows of ITS channel block
// straight into A-fragment registers at kernel start together with everything else the kernel reads (one L2 round trip), the
// hidden activation crosses the waves through LDS, and the prediction eps never leaves the registers: the lane that holds
// eps[row][channel] applies the update to x[row][channel] (and, for the feature DDPM with fixed key points, writes the per-point
// table / concatenation columns of the next step, as update_feat_kernel does).
typedef SlideHeadArgs HeadArgs;  // include/slide_engine.h

template <int K0MAX>  // k0 <= K0MAX (multiple of 32)
__global__ __launch_bounds__(256, 2) void head_update_kernel(HeadArgs a) {
#pragma clang fp contract(off)
  using T = _Float16;
  constexpr int LDX = K0MAX + 8, LDH = 128 + 8;
  __shared__ __attribute__((aligned(16))) T xs[64 * LDX];
  __shared__ __attribute__((aligned(16))) T hs[64 * LDH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int row0 = blockIdx.x * 64;
  const int t = a.t_dev[0], step = a.t_dev[1];
  const uint32_t nonce = (uint32_t)a.t_dev[3];
  const uint32_t eoff = (uint32_t)a.t_dev[4] * (uint32_t)(16 * a.C);
  // ---- every global read of the two layers, issued together
  const int nk0 = a.k0 >> 4;  // 16-deep steps of layer 1
  f16x8 w0[K0MAX / 16];
  {
    const GLOBAL_AS T *wp = gptr<const T>((uint64_t)a.W0) + (size_t)(wave * 32 + col) * a.k0 + half * 8;
#pragma unroll
    for (int s2 = 0; s2 < K0MAX / 16; ++s2)
      if (s2 < nk0) w0[s2] = *(const GLOBAL_AS f16x8 *)(wp + s2 * 16);
  }
  const int cb2 = a.n1c == 2 ? (wave & 1) : 0, rb2 = a.n1c == 2 ? (wave >> 1) : wave;  // layer-2 block of this wave
  const bool l2 = rb2 < 2;
  f16x8 w1[8];
  if (l2) {
    const GLOBAL_AS T *wp = gptr<const T>((uint64_t)a.W1) + (size_t)(cb2 * 32 + col) * 128 + half * 8;
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) w1[s2] = *(const GLOBAL_AS f16x8 *)(wp + s2 * 16);
  }
  {
    const int ppr = a.k0 >> 3;
    for (int i = tid; i < 64 * ppr; i += 256) {
      const int r = i / ppr, pc = i - r * ppr;
      int grow = row0 + r;
      grow = grow < a.rows ? grow : a.rows - 1;
      *reinterpret_cast<u32x4 *>(xs + r * LDX + pc * 8) = *(const GLOBAL_AS u32x4 *)(gptr<const T>((uint64_t)a.X) + (size_t)grow * a.x_ld + pc * 8);
    }
  }
  float bia[16], gam[16], bet[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b4 = *reinterpret_cast<const float4 *>(a.v0 + wave * 32 + 8 * q + 4 * half);
    const float4 g4 = *reinterpret_cast<const float4 *>(a.v0 + 128 + wave * 32 + 8 * q + 4 * half);
    const float4 t4 = *reinterpret_cast<const float4 *>(a.v0 + 256 + wave * 32 + 8 * q + 4 * half);
    bia[4 * q] = b4.x; bia[4 * q + 1] = b4.y; bia[4 * q + 2] = b4.z; bia[4 * q + 3] = b4.w;
    gam[4 * q] = g4.x; gam[4 * q + 1] = g4.y; gam[4 * q + 2] = g4.z; gam[4 * q + 3] = g4.w;
    bet[4 * q] = t4.x; bet[4 * q + 1] = t4.y; bet[4 * q + 2] = t4.z; bet[4 * q + 3] = t4.w;
  }
  float b1v[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b4 = l2 ? *reinterpret_cast<const float4 *>(a.b1 + cb2 * 32 + 8 * q + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);
    b1v[4 * q] = b4.x; b1v[4 * q + 1] = b4.y; b1v[4 * q + 2] = b4.z; b1v[4 * q + 3] = b4.w;
  }
  __syncthreads();
  // ---- layer 1: channel block `wave`, both 32-row blocks; D[channel][row]: lane = row, reg r = channel (r&3)+8(r>>2)+4 half
  f32x16 acc[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < K0MAX / 16; ++s2)
    if (s2 < nk0) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const f16x8 xb = *reinterpret_cast<const f16x8 *>(xs + (rb * 32 + col) * LDX + s2 * 16 + half * 8);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0[s2], xb, acc[rb], 0, 0, 0);
      }
    }
  // bias, GroupNorm(32, 128) = groups of four consecutive channels = the four registers 4q .. 4q+3 of a lane, statistics over
  // the sample's 16 rows = 16 lanes; ReLU; fp16 into LDS [row][channel]
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[4], s = 0.f, ss = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = acc[rb][4 * q + j] + bia[4 * q + j];
        s += v[j];
        ss = fmaf(v[j], v[j], ss);
      }
      s = lane_group_sum<16>(s);
      ss = lane_group_sum<16>(ss);
      const float mean = s * (1.0f / 64.0f);
      const float var = fmaxf(ss * (1.0f / 64.0f) - mean * mean, 0.f);
      const float rstd = __builtin_amdgcn_rsqf(var + GN_EPS);
      f16x4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float g = gam[4 * q + j] * rstd;
        h[j] = (T)fmaxf(fmaf(v[j], g, bet[4 * q + j] - mean * g), 0.f);
      }
      *reinterpret_cast<f16x4 *>(hs + (rb * 32 + col) * LDH + wave * 32 + 8 * q + 4 * half) = h;
    }
  }
  __syncthreads();
  // ---- layer 2 + update
  if (l2) {
    f32x16 e2;
#pragma unroll
    for (int r = 0; r < 16; ++r) e2[r] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const f16x8 hb = *reinterpret_cast<const f16x8 *>(hs + (rb2 * 32 + col) * LDH + s2 * 16 + half * 8);
      e2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[s2], hb, e2, 0, 0, 0);
    }
    const int p = row0 + rb2 * 32 + col;
    if (p < a.rows) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cb2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float ev = e2[r] + b1v[r];
        if (a.eps_out && c < a.eps_ld) a.eps_out[(size_t)p * a.eps_ld + c] = ev;
        if (c >= a.C) continue;
        const int e = p * a.C + c;
        if (a.kind == 1) {
          update_feat_element(e, a.rows, a.C, a.kdim, 0, a.clamp, a.seed_lo, a.seed_hi, a.x, nullptr, a.noise, t, step, nonce, eoff,
                              a.complete_x0, a.kmask, a.keypoint, a.t0, a.t1, a.t2, a.t3, a.t4, a.feat0, a.ldf, a.half_out,
                              a.copies, a.n_copies, ev);
        } else {  // position DDPM: x = (x - c_eps[t] eps) / sqrt_alpha[t] (+ sigma[t] z)   (tables t0, t1, t2)
          float v = (a.x[e] - a.t0[t] * ev) / a.t1[t];
          if (t > 0) {
            const float z = a.noise ? a.noise[(size_t)step * a.rows * 3 + e]
                                    : philox_normal(a.seed_lo, a.seed_hi, (uint32_t)step, (uint32_t)e + (uint32_t)a.t_dev[4] * 48u, nonce);
            v = v + a.t2[t] * z;
          }
          a.x[e] = v;
        }
      }
    }
  }
  advance_t_last_block(a.t_dev, t, step);
}

__global__ void advance_t_kernel(int *t_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    t_dev[0] -= 1;
    t_dev[1] += 1;
  }
}

// batched fp32 transpose through a 32x33 LDS tile (module-level path: NCHW activations <-> the GEMM's row-major
// [pixel][channel] matrices); coalesced on both sides
template <typename TO>
__global__ __launch_bounds__(256) void transpose_kernel(int R, int C, int in_ld, int out_ld, long long in_bs,
                                                        long long out_bs, const float *__restrict__ in,
                                                        TO *__restrict__ out) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  in += (size_t)b * in_bs;
  out += (size_t)b * out_bs;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    if (r < R && c < C) tile[ty + 8 * i][tx] = in[(size_t)r * in_ld + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (r < R && c < C) out[(size_t)c * out_ld + r] = (TO)tile[tx][ty + 8 * i];
  }
}

int run_op(const SlideOp &o, hipStream_t s) {
  switch (o.kind) {
    case SLIDE_OP_GEMM:
      return slide_launch_gemm(o, s);
    case SLIDE_OP_PREP_POINTS:
      if (o.i[3] == SLIDE_PREC_F16)
        hipLaunchKernelGGL(prep_points_kernel<_Float16>, dim3(o.i[0]), dim3(256), 0, s, o.i[1], o.i[2],
                           (const float *)o.p[0], (float *)o.p[1], (_Float16 *)o.p[2], (int *)o.p[3], (float *)o.p[4],
                           (_Float16 *)o.p[5], (const SlidePrepCopy *)o.p[6], o.i[4], (float *)o.p[7]);
      else
        hipLaunchKernelGGL(prep_points_kernel<float>, dim3(o.i[0]), dim3(256), 0, s, o.i[1], o.i[2],
                           (const float *)o.p[0], (float *)o.p[1], (float *)o.p[2], (int *)o.p[3], (float *)o.p[4],
                           (float *)o.p[5], (const SlidePrepCopy *)o.p[6], o.i[4], (float *)o.p[7]);
      break;
    case SLIDE_OP_ASSEMBLE_SA:
    case SLIDE_OP_ASSEMBLE_FP: {
      const bool fp = o.kind == SLIDE_OP_ASSEMBLE_FP;
      // bulk (whole 16-byte pieces of the gathered rows) and tail (coordinate pieces) blocks, see the kernel.
      // i[6] = c_begin (multiple of 32): only columns >= c_begin are produced, into rows of i[7] elements
      const int esz = o.i[5] == SLIDE_PREC_F16 ? 2 : 4;
      const int c_begin = o.i[6], ld_out = o.i[6] ? o.i[7] : o.i[3];
      const int nch = o.i[3] / 8, nbulk = (esz * o.i[2] % 16 == 0) ? o.i[1] / 8 : 0, ntail = nch - nbulk;
      // the element-wise pieces start at column 8 nbulk: with c_begin beyond it they would be stored in front of their row
      if (c_begin < 0 || c_begin % 8 || c_begin > nbulk * 8) return -3;
      const int nb_eff = nbulk - c_begin / 8 > 0 ? nbulk - c_begin / 8 : 0;
      int nch_log2 = 0;
      while ((1 << nch_log2) < nb_eff) ++nch_log2;
      const int bulk_blocks = nb_eff ? (((16 * o.i[4]) << nch_log2) + 255) / 256 : 0;
      const int tail_blocks = (16 * o.i[4] * ntail + 255) / 256;
      const dim3 g(o.i[0], bulk_blocks + tail_blocks), blk(256);
      const float *kd2 = fp ? (const float *)o.p[3] : nullptr;
      void *dst = fp ? o.p[4] : o.p[3];
#define ASM(TT, FPB)                                                                                                  \
  hipLaunchKernelGGL((assemble_kernel<TT, FPB>), g, blk, 0, s, o.i[1], o.i[2], o.i[3], o.i[4], nch_log2, bulk_blocks, c_begin, ld_out, (const float *)o.p[0], \
                     (const TT *)o.p[1], (const int *)o.p[2], kd2, (TT *)dst)
      if (o.i[5] == SLIDE_PREC_F16) { if (fp) ASM(_Float16, true); else ASM(_Float16, false); }
      else { if (fp) ASM(float, true); else ASM(float, false); }
#undef ASM
      break;
    }
    case SLIDE_OP_FINALIZE_GN:
      hipLaunchKernelGGL(finalize_gn_kernel, dim3((o.i[0] * o.i[1] + 255) / 256), dim3(256), 0, s, o.i[0], o.i[1],
                         o.i[2], o.f[0], (const float *)o.p[0], (const float *)o.p[1], (const int *)o.p[2],
                         (const int *)o.p[3], (const int *)o.p[4], (const float *)o.p[5], (const float *)o.p[6],
                         (float *)o.p[7], (float *)o.p[8]);
      break;
    case SLIDE_OP_ATTN_COMBINE: {
      const int n = o.i[0] * o.i[1];
      const dim3 g((n + 255) / 256), blk(256);
#define ATTN(KK, TT)                                                                                              \
  hipLaunchKernelGGL((attn_combine_kernel<KK, TT>), g, blk, 0, s, o.i[0], o.i[1], o.i[2], o.i[3], o.i[4],         \
                     (const TT *)o.p[0], (const TT *)o.p[1], (TT *)o.p[2])
      if (o.i[5] == 16 && o.i[6] == SLIDE_PREC_F16) ATTN(16, _Float16);
      else if (o.i[5] == 16) ATTN(16, float);
      else if (o.i[5] == 8 && o.i[6] == SLIDE_PREC_F16) ATTN(8, _Float16);
      else if (o.i[5] == 8) ATTN(8, float);
      else return -5;
#undef ATTN
      break;
    }
    case SLIDE_OP_COPY_COLS: {
      if (o.i[0] <= 0 || o.i[1] <= 0) break;  // nothing to copy (a zero-sized grid is a launch error)
      const dim3 g((o.i[0] * o.i[1] + 255) / 256), blk(256);
#define CPY(TS, TD)                                                                                               \
  hipLaunchKernelGGL((copy_cols_kernel<TS, TD>), g, blk, 0, s, o.i[0], o.i[1], o.i[2], o.i[3], (const TS *)o.p[0], \
                     (TD *)o.p[1])
      if (o.i[4] && o.i[5]) CPY(_Float16, _Float16);
      else if (o.i[4]) CPY(_Float16, float);
      else if (o.i[5]) CPY(float, _Float16);
      else CPY(float, float);
#undef CPY
      break;
    }
    case SLIDE_OP_TEMB:
      hipLaunchKernelGGL(temb_kernel, dim3(o.i[0]), dim3(256), (size_t)o.i[1] * 9 * sizeof(float), s, o.i[1], o.i[2],
                         (const float *)o.p[0], (const int *)o.p[1], (const float *)o.p[9], (const float *)o.p[2],
                         (const float *)o.p[3], (const float *)o.p[4], (const float *)o.p[5], (const float *)o.p[6],
                         (const float *)o.p[7], (float *)o.p[8]);
      break;
    case SLIDE_OP_COND:
      hipLaunchKernelGGL(cond_kernel, dim3(o.i[0]), dim3(256), (size_t)o.i[1] * sizeof(float), s, o.i[1], o.i[2],
                         (const int64_t *)o.p[0], (const float *)o.p[1], (const float *)o.p[2], (const float *)o.p[3],
                         (float *)o.p[4]);
      break;
    case SLIDE_OP_UPDATE_POS:
      hipLaunchKernelGGL(update_pos_kernel, dim3((o.i[0] + 255) / 256), dim3(256), 0, s, o.i[0], o.i[1], (uint32_t)o.i[2],
                         (uint32_t)o.i[3], (float *)o.p[0], (const float *)o.p[1], (const float *)o.p[2],
                         (int *)o.p[3], (const float *)o.p[4], (const float *)o.p[5], (const float *)o.p[6]);
      break;
    case SLIDE_OP_UPDATE_FEAT:
      hipLaunchKernelGGL(update_feat_kernel<SLIDE_UPDATE_FEAT_EPT>,
                         dim3((o.i[0] + 4 * SLIDE_UPDATE_FEAT_EPT - 1) / (4 * SLIDE_UPDATE_FEAT_EPT), (o.i[1] + 63) / 64), dim3(256), 0, s, o.i[0], o.i[1],
                         o.i[2], o.i[5], o.f[0], (uint32_t)o.i[3], (uint32_t)o.i[4], (float *)o.p[0], (const float *)o.p[1],
                         (const float *)o.p[2], (int *)o.p[3], (const float *)o.p[4], (const float *)o.p[5],
                         (const float *)o.p[6], (const float *)o.p[7], (const float *)o.p[8], (const float *)o.p[9],
                         (const float *)o.p[10], (const float *)o.p[11], o.p[12], o.i[6], o.i[7],
                         (const SlidePrepCopy *)o.p[13], o.i[8]);
      break;
#ifndef SLIDE_EXPERIMENTS
    case SLIDE_OP_HEAD_UPDATE:
    case SLIDE_OP_GEMM_CHAIN:
      return SLIDE_ST_EXPERIMENT;
#else
    case SLIDE_OP_GEMM_CHAIN:
      return slide_launch_gemm_chain(o, s);
    case SLIDE_OP_HEAD_UPDATE: {
      const SlideHeadArgs *h = (const SlideHeadArgs *)o.p[0];  // HOST pointer, kept alive by the plan
      if (!h || h->rows <= 0 || h->rows % 16 || h->k0 % 32 || h->k0 <= 0 || h->k0 > 160 || h->x_ld < h->k0 || h->x_ld % 8 ||
          (h->n1c != 1 && h->n1c != 2) || !h->X || !h->W0 || !h->W1 || !h->v0 || !h->b1 || !h->x || !h->t_dev ||
          (h->kind != 0 && h->kind != 1) || h->C > 32 * h->n1c)
        return -3;
      const int grid = (h->rows + 63) / 64;
      if (h->k0 <= 96) hipLaunchKernelGGL(head_update_kernel<96>, dim3(grid), dim3(256), 0, s, *h);
      else hipLaunchKernelGGL(head_update_kernel<160>, dim3(grid), dim3(256), 0, s, *h);
      break;
    }
#endif
    case SLIDE_OP_POINT_CHAIN:
      return slide_launch_point_chain(o, s);
    case SLIDE_OP_GEMM_ATTEND:
      return slide_launch_gemm_attend(o, s);
    case SLIDE_OP_ATTN_TAIL:
      return ((int)o.f[1] & 8) ? slide_launch_attn_tail_split(o, s) : slide_launch_attn_tail(o, s);
    case SLIDE_OP_GEMM_GX:
      return (int)o.f[0] == 3 ? slide_launch_gemm_gxs(o, s) : slide_launch_gemm_gx(o, s);
    case SLIDE_OP_GEMM_GX_DUAL:
      return slide_launch_gemm_gx_dual(o, s);
    case SLIDE_OP_PAIR_NORM:
      return slide_launch_pair_norm(o, s);
    case SLIDE_OP_PP_STAGE:
#ifdef SLIDE_EXPERIMENTS
      return slide_launch_pp_stage(o, s);
#else
      return SLIDE_ST_EXPERIMENT;  // (measured slower, opt-in: experiments/pp_stage.hip)
#endif
    case SLIDE_OP_PAIR_FIRST:
      return slide_launch_pair_first(o, s);
    case SLIDE_OP_SA_CHAIN:
      return slide_launch_sa_chain(o, s);
    case SLIDE_OP_SA_CHAIN_P:
      return slide_launch_sa_chain_p(o, s);
    case SLIDE_OP_BLOCK_BODY:
#ifdef SLIDE_EXPERIMENTS
      return slide_launch_block_body(o, s);
#else
      return SLIDE_ST_EXPERIMENT;  // (opt-in since round 5: block_body.hip is part of the experiments build)
#endif
    case SLIDE_OP_TRANSPOSE:  // i: B, R, C, in_ld, out_ld, in_batch_stride, out_batch_stride, out_is_fp16   p: in, out
      // (an empty or oversized grid is a launch error; a leading dimension below the row length overlaps rows)
      if (o.i[0] <= 0 || o.i[0] > 65535 || o.i[1] <= 0 || (o.i[1] + 31) / 32 > 65535 || o.i[2] <= 0 || o.i[3] < o.i[2] || o.i[4] < o.i[1] ||
          !o.p[0] || !o.p[1])
        return -3;
      if (o.i[7])  // fp16 destination (module-level throughput mode)
        hipLaunchKernelGGL(transpose_kernel<_Float16>, dim3((o.i[2] + 31) / 32, (o.i[1] + 31) / 32, o.i[0]), dim3(256), 0, s,
                           o.i[1], o.i[2], o.i[3], o.i[4], (long long)o.i[5], (long long)o.i[6], (const float *)o.p[0],
                           (_Float16 *)o.p[1]);
      else
        hipLaunchKernelGGL(transpose_kernel<float>, dim3((o.i[2] + 31) / 32, (o.i[1] + 31) / 32, o.i[0]), dim3(256), 0, s,
                           o.i[1], o.i[2], o.i[3], o.i[4], (long long)o.i[5], (long long)o.i[6], (const float *)o.p[0],
                           (float *)o.p[1]);
      break;
    case SLIDE_OP_GROUPNORM_NCHW:  // i: B, C, HW, G, n_norm, relu   p: x, gamma, beta, y
      // (G = 0 divides by zero on the device; n_norm % G != 0 or n_norm > C normalises a span that is not the groups')
      if (o.i[0] <= 0 || o.i[0] > 65535 || o.i[1] <= 0 || o.i[2] <= 0 || o.i[3] < 1 || o.i[4] <= 0 || o.i[4] > o.i[1] || o.i[4] % o.i[3] ||
          !o.p[0] || !o.p[1] || !o.p[2] || !o.p[3])
        return -3;
      hipLaunchKernelGGL(group_norm_nchw_kernel, dim3(o.i[3] + (o.i[4] < o.i[1] ? 1 : 0), o.i[0]), dim3(256), 0, s, o.i[1],
                         o.i[2], o.i[3], o.i[4], o.i[5], (const float *)o.p[0], (const float *)o.p[1],
                         (const float *)o.p[2], (float *)o.p[3]);
      break;
    case SLIDE_OP_ADVANCE_T:
      hipLaunchKernelGGL(advance_t_kernel, dim3(1), dim3(64), 0, s, (int *)o.p[0]);
      break;
    default:
      if ((o.kind >= SLIDE_OP_ROWS_FROM_NCX && o.kind <= SLIDE_OP_ROWS_GN_JOINT) || o.kind == SLIDE_OP_ROWS_PAIR_EXPAND)
        return slide_launch_rows_op(o, s);
      return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int slide_run_ops(const SlideOp *ops, int n, slide_stream_t stream) { return slide_run_ops2(ops, n, stream, stream); }

// Two-lane replay: op.i[10] selects the lane (stream); SLIDE_OP_SYNC(from, to) makes lane `to` wait for everything
// issued so far on lane `from` (event record + stream wait -> a plain edge when captured into a hipGraph).
int slide_run_ops2(const SlideOp *ops, int n, slide_stream_t stream0, slide_stream_t stream1) {
  hipStream_t ss[2] = {(hipStream_t)stream0, (hipStream_t)stream1};
  // fork / join events of the two-lane plans: one small pool per host thread (events belong to the device that was
  // current when they were created; a thread drives one device)
  static thread_local hipEvent_t pool[256];
  static thread_local int pool_n = 0, pool_next = 0;
  for (int i = 0; i < n; ++i) {
    const SlideOp &o = ops[i];
    if (o.kind == SLIDE_OP_SYNC) {
      const int from = o.i[0] & 1, to = o.i[1] & 1;
      if (ss[from] == ss[to]) continue;
      if (pool_n < 256) {
        if (hipEventCreateWithFlags(&pool[pool_n], hipEventDisableTiming) != hipSuccess) return -9;
        ++pool_n;
      }
      hipEvent_t ev = pool[pool_next % pool_n];
      pool_next = (pool_next + 1) % 256;
      hipError_t e = hipEventRecord(ev, ss[from]);
      if (e == hipSuccess) e = hipStreamWaitEvent(ss[to], ev, 0);
      if (e != hipSuccess) return (int)e;
      continue;
    }
    const int st = run_op(o, ss[o.i[10] & 1]);
    if (st != 0) return st > 0 ? st : st * 1000 - i;
  }
  return 0;
}

// `reps` eager replays of one plan in a single call: a host thread per chain can keep its stream fed without returning
// to the interpreter between steps (plans advance their own device-side timestep).  Thread-safe for plans without
// SLIDE_OP_SYNC on distinct streams once every kernel has been launched at least once (first-use attribute calls).
int slide_run_ops_repeat(const SlideOp *ops, int n, slide_stream_t stream0, slide_stream_t stream1, int reps) {
  for (int r = 0; r < reps; ++r) {
    const int st = slide_run_ops2(ops, n, stream0, stream1);
    if (st != 0) return st;
  }
  return 0;
}

// `reps` steps of several independent chains from ONE host thread, round-robin: step r of every chain is issued before
// step r + 1 of any (chain c replays ops[c][0..n[c]) on streams[c]; single-lane plans).
int slide_run_chains(const SlideOp *const *ops, const int *n, const slide_stream_t *streams, int n_chains, int reps) {
  for (int r = 0; r < reps; ++r)
    for (int c = 0; c < n_chains; ++c) {
      const int st = slide_run_ops2(ops[c], n[c], streams[c], streams[c]);
      if (st != 0) return st;
    }
  return 0;
}

// The same with chain c stepping only on every every[c]-th round (a chain over a multiple of the common batch advances once per
// `every` rounds of the others: same shapes per unit time, fewer dependent launches on the critical path).
int slide_run_chains_every(const SlideOp *const *ops, const int *n, const slide_stream_t *streams, const int *every, int n_chains,
                           int reps) {
  for (int r = 0; r < reps; ++r)
    for (int c = 0; c < n_chains; ++c) {
      if (every[c] > 1 && r % every[c] != 0) continue;
      const int st = slide_run_ops2(ops[c], n[c], streams[c], streams[c]);
      if (st != 0) return st;
    }
  return 0;
}

// Eager replay with a HIP event between consecutive launches (recorded on the launch stream): ms_out[i] = device
// time of ops[i].  Used by bench.py for the per-kernel roofline figure; not used on the timed path.
int slide_run_ops_timed(const SlideOp *ops, int n, slide_stream_t stream, float *ms_out) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0 || n > 4096) return -6;
  hipEvent_t *ev = new hipEvent_t[n + 1];
  int st = 0;
  for (int i = 0; i <= n; ++i) st |= (int)hipEventCreate(&ev[i]);
  if (st == 0) st = (int)hipEventRecord(ev[0], s);
  for (int i = 0; i < n && st == 0; ++i) {
    if (ops[i].kind != SLIDE_OP_SYNC) st = run_op(ops[i], s);  // single-stream replay: syncs are no-ops
    if (st == 0) st = (int)hipEventRecord(ev[i + 1], s);
  }
  if (st == 0) st = (int)hipEventSynchronize(ev[n]);
  for (int i = 0; i < n && st == 0; ++i) st = (int)hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
  for (int i = 0; i <= n; ++i) (void)hipEventDestroy(ev[i]);
  delete[] ev;
  return st;
}

int slide_graph_begin(slide_stream_t stream) {
  return (int)hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal);
}
int slide_graph_end(slide_stream_t stream, void **graph_exec_out) {
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &g);
  if (e != hipSuccess) return (int)e;
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return (int)e;
  *graph_exec_out = (void *)ex;
  return 0;
}
int slide_graph_launch(void *graph_exec, slide_stream_t stream) {
  return (int)hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
}
int slide_graph_destroy(void *graph_exec) { return (int)hipGraphExecDestroy((hipGraphExec_t)graph_exec); }

int slide_stream_create_cu_mask(const uint32_t *mask, int n_words, slide_stream_t *stream_out) {
  if (!mask || n_words <= 0 || !stream_out) return -3;
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, mask);
  *stream_out = (slide_stream_t)st;
  return (int)e;
}
int slide_stream_destroy(slide_stream_t stream) { return (int)hipStreamDestroy((hipStream_t)stream); }

int slide_event_create(void **ev) {
  hipEvent_t e;
  const hipError_t st = hipEventCreate(&e);
  *ev = (void *)e;
  return (int)st;
}
int slide_event_record(void *ev, slide_stream_t stream) { return (int)hipEventRecord((hipEvent_t)ev, (hipStream_t)stream); }
int slide_event_elapsed_ms(void *start, void *stop, float *ms) {
  hipError_t st = hipEventSynchronize((hipEvent_t)stop);
  if (st != hipSuccess) return (int)st;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}
int slide_event_destroy(void *ev) { return (int)hipEventDestroy((hipEvent_t)ev); }

int slide_sizeof_epi(void) { return (int)sizeof(SlideEpi); }
int slide_sizeof_op(void) { return (int)sizeof(SlideOp); }

}  // extern "C"
