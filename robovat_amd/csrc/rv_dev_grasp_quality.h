// rv_dev_grasp_quality.h -- the grasp-quality network of rv_grasp_quality (include/rovat.h): the forward
// pass that turns the grasp-centred depth crop of a candidate (rv_grasp_crops) and its grasp depth into one logit.
// A stand-alone kernel beside the env program, like rv_dev_cem.h; it includes rv_dev_env.h for rv_fma and RV_DEV only.
//
// The network, per sample (x [h][w] the crop, z the grasp depth; sizes from rv_grasp_quality_model):
//   a  = (x - im_mean) * im_inv_std                      two float32 operations, each rounded on its own
//   u  = (z - z_mean) * z_inv_std
//   c1 = pool2(relu(conv5x5_same(a;  1 -> C1)))          [C1][h/2][w/2]
//   c2 = pool2(relu(conv3x3_same(c1; C1 -> C2)))         [C2][h/4][w/4]
//   f1 = relu(fc(flatten(c2) -> F1))                     flatten is channel-major: index ch (h/4)(w/4) + row (w/4) + col
//   p  = relu(fc(u -> P))
//   f2 = relu(fc(concat(f1, p) -> F2))
//   logit = fc(f2 -> 1)
// "same" pads the NORMALISED image (and c1) with zeros; relu(v) = v > 0 ? v : 0.0f (so relu(NaN) = relu(-0) = +0);
// pool2 is the maximum of the 2 x 2 window taken after relu, m = v00; m = v01 > m ? v01 : m; then v10, v11.
//
// Arithmetic.  Every dot product is ONE float32 FMA chain: acc = bias; acc = fma(in_k, w_k, acc) for the terms in
// ascending input index k -- for the convolutions k = (channel, tap row, tap column), for fc1 the flatten index, for fc2
// f1 then p --, one rounding per term, no partial sums, no reassociation.  That is rv_fma of rv_dev_math.h, and it is what
// v_mfma_f32_16x16x4_f32 computes along k (D = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1, fma(a_k0, b_k0, C)))), so
// the layers on the matrix cores and the VALU layers share one definition, and tests/grasp_quality_host.py restates all of
// it in float32 NumPy; the GPU tests compare bit for bit.  Zero operands stand in for what is not there: the zero border of
// "same", and -- as B columns and as A rows -- output channels past C2 / F1 / F2 and pool windows past the last one of a
// crop; those results are never stored.  No K dimension is padded: 9 C1, C2 (h/4)(w/4) and F1 + P are multiples of 4
// because C1, C2, F1 and P are.  The logit (K = F2) is a VALU chain.
//
// Weight blob (one float32 buffer, rv_grasp_quality_weight_count floats), in this order:
//   conv1.weight [C1][5][5]      conv1.bias [C1]
//   conv2.weight [9 C1][C2]      K-major: row k = ci 9 + ky 3 + kx          conv2.bias [C2]
//   fc1.weight   [C2 (h/4)(w/4)][F1]   K-major                              fc1.bias [F1]
//   pose.weight  [P]             pose.bias [P]
//   fc2.weight   [F1 + P][F2]    K-major                                    fc2.bias [F2]
//   out.weight   [F2]            out.bias [1]
// K-major: the 16 lanes of a B fragment row read 16 consecutive floats.
//
// Shape: one launch, one workgroup of four waves per RV_GQ_BATCH = 8 consecutive samples, everything between the crop and
// the logit in LDS (dynamic: at the default sizes 5 KB padded image, 20 KB padded c1, 32 KB for the c2 of the 8 samples,
// 5 KB for the head, 9 KB for conv2's weights, copied there once per workgroup: 73 KB, two workgroups per CU, and 78 KB
// for the largest model).  Per sample: the image is normalised into a zero-bordered LDS tile; conv1 is a VALU loop, a
// lane per pooled pixel holding its 6 x 6 input patch in registers, channels in a loop whose 25 weights and bias are
// wave-uniform scalar loads; conv2 is an implicit GEMM on v_mfma_f32_16x16x4_f32 with M = 16 pre-pool pixels ordered so
// that a lane's four accumulator registers are one pool window, N = 16 output channels, K = 9 C1 gathered from the
// zero-bordered c1 by a per-lane table of nine offsets, four M tiles (independent accumulators) per B fragment.  Then fc1
// with the batch as M (8 of the tile's 16 rows; the other 8 repeat row 0 and are dropped), so that its weights (256 KB at
// the default sizes, streamed from L2) are read once per 8 samples, fc2 the same way, the pose stream and the logit as
// VALU chains.  A batch of 16 fills the M tile but its 110 KB of LDS leave one workgroup, one wave per SIMD, on a CU:
// measured 2.06 ms against this shape's time in DESIGN.md §21.  No atomics; the logits leave by ordinary vector stores;
// every global index is a size_t.
#ifndef RV_DEV_GRASP_QUALITY_H_
#define RV_DEV_GRASP_QUALITY_H_
#include "rv_dev_env.h"

#define RV_GQ_BATCH 8
#define RV_GQ_TPB 256

namespace rv {
struct GqArgs {
  const float* images;      // [rows][h][w]
  const float* depths;      // [rows]
  float* logits;            // [rows]
  int h, w, c1, c2, f1, f2, p;
  float im_mean, im_inv_std, z_mean, z_inv_std;
  uint32_t rows;
};
// offsets (in floats) into the weight blob and into LDS, for the host and the device alike
struct GqLayout {
  int H1, W1, RS1, PL1, IW, IH, P2, K1, S2, KC, SC, SF;
  long long c1w, c1b, c2w, c2b, f1w, f1b, pw, pb, f2w, f2b, ow, ob, count;
  int l_img, l_c1, l_c2, l_cat, l_f2, l_w2, l_floats;
};
__host__ __device__ inline GqLayout gq_layout(int h, int w, int c1, int c2, int f1, int f2, int p) {
  GqLayout L;
  L.H1 = h / 2; L.W1 = w / 2; L.RS1 = L.W1 + 2; L.PL1 = (L.H1 + 2) * L.RS1; L.IW = w + 4; L.IH = h + 4;
  L.P2 = (h / 4) * (w / 4); L.K1 = c2 * L.P2; L.S2 = L.K1 + 4; L.KC = f1 + p; L.SC = L.KC + 4; L.SF = f2 + 4;
  L.c1w = 0; L.c1b = L.c1w + 25LL * c1; L.c2w = L.c1b + c1; L.c2b = L.c2w + 9LL * c1 * c2; L.f1w = L.c2b + c2;
  L.f1b = L.f1w + (long long)L.K1 * f1; L.pw = L.f1b + f1; L.pb = L.pw + p; L.f2w = L.pb + p;
  L.f2b = L.f2w + (long long)L.KC * f2; L.ow = L.f2b + f2; L.ob = L.ow + f2; L.count = L.ob + 1;
  L.l_img = 0; L.l_c1 = L.l_img + L.IH * L.IW; L.l_c2 = L.l_c1 + c1 * L.PL1; L.l_cat = L.l_c2 + RV_GQ_BATCH * L.S2;
  L.l_f2 = L.l_cat + RV_GQ_BATCH * L.SC; L.l_w2 = L.l_f2 + RV_GQ_BATCH * L.SF; L.l_floats = L.l_w2 + 9 * c1 * c2;
  return L;
}

typedef float gq_f32x4 __attribute__((ext_vector_type(4)));
RV_DEV float gq_relu(float v) { return v > 0.0f ? v : 0.0f; }
RV_DEV float gq_pool(float v00, float v01, float v10, float v11) {
  float m = gq_relu(v00);
  const float b = gq_relu(v01), c = gq_relu(v10), d = gq_relu(v11);
  m = b > m ? b : m; m = c > m ? c : m; m = d > m ? d : m;
  return m;
}

// out[m][n] = relu(bias[n] + the k-ordered FMA chain of A[m][k] B[k][n]) for the 16 rows of A: A in LDS with row stride
// sa, B K-major [K][N] in global memory, K a multiple of 4; a wave per 16 columns.  The M = 16 tile holds the batch's
// RV_GQ_BATCH rows; the rest of it is computed on copies of row 0 and thrown away
RV_DEV void gq_fc(const float* A, int sa, const float* B, const float* bias, int K, int N, float* out, int so, int wave, int lane) {
  const int m16 = lane & 15, kq = lane >> 4;
  for (int nt = wave; nt * 16 < N; nt += RV_GQ_TPB / 64) {
    const int n = nt * 16 + m16;
    const bool nok = n < N;
    const float b0 = nok ? bias[n] : 0.0f;
    gq_f32x4 acc = {b0, b0, b0, b0};
    const float* ap = A + (m16 < RV_GQ_BATCH ? m16 : 0) * sa + kq;      // (rows past the batch repeat row 0 and are dropped)
    const float* bp = B + (size_t)kq * (size_t)N + (size_t)(nok ? n : 0);
    // (sixteen k steps of loads ahead of their sixteen dependent MFMAs: one trip to L2 per 64 k)
    int k = 0;
    for (; k + 64 <= K; k += 64) {
      float av[16], bv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        av[i] = ap[k + 4 * i];
        const float t = bp[(size_t)(k + 4 * i) * (size_t)N];
        bv[i] = nok ? t : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc, 0, 0, 0);
    }
    for (; k < K; k += 4) {
      const float t = bp[(size_t)k * (size_t)N];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], nok ? t : 0.0f, acc, 0, 0, 0);
    }
    if (nok)
      for (int r = 0; r < 4; ++r)
        if (4 * kq + r < RV_GQ_BATCH) out[(4 * kq + r) * so + n] = gq_relu(acc[r]);
  }
}
}  // namespace rv

// (the blob is a __restrict__ parameter of its own: the kernel never writes it, so wave-uniform reads of it are scalar loads)
__global__ __launch_bounds__(RV_GQ_TPB, 2) void k_grasp_quality(rv::GqArgs a, const float* __restrict__ W) {
  using namespace rv;
  extern __shared__ __align__(16) float gq_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = a.h, w = a.w, C1 = a.c1, C2 = a.c2, F1 = a.f1, F2 = a.f2, P = a.p;
  const GqLayout L = gq_layout(h, w, C1, C2, F1, F2, P);
  float* imgs = gq_lds + L.l_img;
  float* c1s = gq_lds + L.l_c1;
  float* c2s = gq_lds + L.l_c2;
  float* cat = gq_lds + L.l_cat;
  float* f2s = gq_lds + L.l_f2;
  float* w2s = gq_lds + L.l_w2;
  // the zero borders of the image and of c1 are written here once, and the c2 rows of samples past the last one are zero
  for (int i = tid; i < L.l_w2; i += RV_GQ_TPB) gq_lds[i] = 0.0f;
  for (int i = tid; i < 9 * C1 * C2; i += RV_GQ_TPB) w2s[i] = W[L.c2w + i];      // conv2's weights, K-major as they are
  __syncthreads();
  const size_t row0 = (size_t)blockIdx.x * RV_GQ_BATCH;
  const int nb = (size_t)a.rows - row0 < (size_t)RV_GQ_BATCH ? (int)((size_t)a.rows - row0) : RV_GQ_BATCH;
  const int m16 = lane & 15, kq = lane >> 4;
  // conv2's gather: the nine k of a group of four input channels that this lane supplies (k = 4 j + kq of 36)
  int off[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int kl = 4 * j + kq, ci = kl / 9, tap = kl - 9 * ci;
    off[j] = ci * L.PL1 + (tap / 3) * L.RS1 + tap % 3;
  }
  const int W2 = w / 4, tiles = (L.P2 + 3) / 4;

  for (int m = 0; m < nb; ++m) {
    // -- the normalised image into its zero-bordered tile
    const float* img = a.images + (row0 + (size_t)m) * (size_t)(h * w);
    for (int i = tid; i < h * w; i += RV_GQ_TPB) {
      const int y = i / w, x = i - y * w;
      const float v = img[i] - a.im_mean;
      imgs[(y + 2) * L.IW + x + 2] = v * a.im_inv_std;
    }
    __syncthreads();
    // -- conv1 5x5 + relu + pool2: a lane per pooled pixel, channels in a loop with wave-uniform weights
    for (int pix = tid; pix < L.H1 * L.W1; pix += RV_GQ_TPB) {
      const int py = pix / L.W1, px = pix - py * L.W1;
      float in[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) in[r][c] = imgs[(2 * py + r) * L.IW + 2 * px + c];
      for (int c = 0; c < C1; ++c) {
        const float* wc = W + L.c1w + (size_t)c * 25;
        const float b = W[L.c1b + c];
        float v00 = b, v01 = b, v10 = b, v11 = b;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
          for (int kx = 0; kx < 5; ++kx) {
            const float wt = wc[ky * 5 + kx];
            v00 = rv_fma(in[ky][kx], wt, v00);
            v01 = rv_fma(in[ky][kx + 1], wt, v01);
            v10 = rv_fma(in[ky + 1][kx], wt, v10);
            v11 = rv_fma(in[ky + 1][kx + 1], wt, v11);
          }
        c1s[c * L.PL1 + (py + 1) * L.RS1 + px + 1] = gq_pool(v00, v01, v10, v11);
      }
    }
    __syncthreads();
    // -- conv2 3x3 + relu + pool2 as an implicit GEMM: M tile = four pool windows x their four pixels
    float* c2m = c2s + m * L.S2;
    for (int nt = 0; nt * 16 < C2; ++nt) {
      const int n = nt * 16 + m16;
      const bool nok = n < C2;
      const float b0 = nok ? W[L.c2b + n] : 0.0f;
      const float* wk0 = w2s + kq * C2 + (nok ? n : 0);
      for (int t0 = wave; t0 < tiles; t0 += 16) {
        int abase[4]; bool aok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int q = (t0 + 4 * u) * 4 + (m16 >> 2);
          aok[u] = q < L.P2;
          const int py = q / W2, px = q - py * W2;
          abase[u] = aok[u] ? (2 * py + ((m16 >> 1) & 1)) * L.RS1 + 2 * px + (m16 & 1) : 0;
        }
        gq_f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = gq_f32x4{b0, b0, b0, b0};
        for (int cg = 0; cg < C1 / 4; ++cg) {
          const float* wk = wk0 + cg * 36 * C2;
          const float* ck = c1s + cg * 4 * L.PL1;
#pragma unroll
          for (int j = 0; j < 9; ++j) {
            const float bt = wk[4 * j * C2];
            const float bv = nok ? bt : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float at = ck[abase[u] + off[j]];
              const float av = aok[u] ? at : 0.0f;
              acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[u], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int q = (t0 + 4 * u) * 4 + kq;      // the pool window in this lane's four accumulator registers
          if (nok && q < L.P2) c2m[n * L.P2 + q] = gq_pool(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
        }
      }
    }
    // (the next sample's image is written after every wave has left conv1, its c1 after every wave has left this conv2:
    // the two barriers above are between them)
  }
  __syncthreads();
  // -- fc1 over the batch, and the pose stream beside it
  gq_fc(c2s, L.S2, W + L.f1w, W + L.f1b, L.K1, F1, cat, L.SC, wave, lane);
  for (int i = tid; i < RV_GQ_BATCH * P; i += RV_GQ_TPB) {
    const int m = i / P, j = i - m * P;
    float v = 0.0f;
    if (m < nb) {
      const float u = (a.depths[row0 + (size_t)m] - a.z_mean) * a.z_inv_std;
      v = gq_relu(rv_fma(u, W[L.pw + j], W[L.pb + j]));
    }
    cat[m * L.SC + F1 + j] = v;
  }
  __syncthreads();
  gq_fc(cat, L.SC, W + L.f2w, W + L.f2b, L.KC, F2, f2s, L.SF, wave, lane);
  __syncthreads();
  if (tid < nb) {
    float acc = W[L.ob];
    for (int k = 0; k < F2; ++k) acc = rv_fma(f2s[tid * L.SF + k], W[L.ow + k], acc);
    a.logits[row0 + (size_t)tid] = acc;
  }
}
#endif
