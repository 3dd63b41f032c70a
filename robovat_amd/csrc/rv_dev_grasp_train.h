// rv_dev_grasp_train.h -- a training step of the grasp-quality network of rv_dev_grasp_quality.h on the device
// (rv_grasp_quality_forward_train, rv_grasp_quality_backward, rv_adam_step; include/rovat.h).
// Stand-alone kernels beside the env program; rv_dev_env.h is included for rv_fma and RV_DEV only, and
// rv_dev_grasp_quality.h for the blob's layout (gq_layout), gq_relu and gq_fc, which k_grasp_quality keeps as they are.
//
// The loss is not here: the forward entry returns logits, the caller turns them into dL/dlogit per sample (any loss; no
// exponential runs in a kernel), and the backward entry takes that vector g[b], b = 0 .. m-1.
//
// FORWARD (k_gq_train_forward).  k_grasp_quality's arithmetic and shape, chain for chain, so the logits are its logits bit
// for bit; beside them it writes, per sample, a row of the workspace (GtLayout, floats):
//   c1 [C1][h/2][w/2], c2 [C2][h/4][w/4]   the pooled activations
//   i1, i2 (the same shapes)               which position of its 2 x 2 window the pool chose, as the float 0, 1, 2 or 3 =
//                                          2 row + column, in gq_pool's order: v00, then v01, v10, v11 each under a strict
//                                          >, so the first of equal maxima wins and an all-zero window chooses 0
//   cat = f1 [F1] then p [P], f2 [F2], u   the head's activations and the normalised grasp depth
// and leaves room for what the backward pass writes: g (its copy of g[b]), dz2 [F2], dzc [F1 + P] and the per-sample
// partial sums s2 [9 C1][C2], s2b [C2], s1 [C1][25], s1b [C1].
//
// BACKWARD.  Every gradient is a float32 chain from +0 whose order is a function of the shapes alone -- never of the grid,
// of a tile, of m's divisibility or of the arrival order of waves; there are no atomics.  "fma chain of (a_k, b_k)" is
// acc = +0; acc = rv_fma(a_k, b_k, acc) in the order given; "sum chain" is acc = +0; acc = acc + t_k, each sum rounded.
// relu passes a gradient where the STORED activation is > 0, a pool window passes it to the position the forward pass
// chose and only when the pooled value is > 0; what is not passed is +0.
//  per sample b (k_gq_train_backward_sample, one workgroup per sample):
//   dz2[o]  = f2[o] > 0 ? rv_fma(g, out.w[o], +0) : +0                                           o < F2
//   dzc[i]  = cat[i] > 0 ? fma chain over o ascending of (dz2[o], fc2.w[o][i]) : +0              i < F1 + P
//             (its first F1 entries are the gradient at fc1's pre-activation, the other P at the pose layer's)
//   g2[k]   = c2[k] > 0 ? fma chain over o ascending of (dzc[o], fc1.w[o][k]) : +0               k < C2 (h/4)(w/4), o < F1
//             (the gradient at conv2's output, at the chosen position of window k; flatten order)
//   s2[ci][ky][kx][co] = fma chain over the windows q of channel co in row-major order, those with c2 > 0 only, of
//             (g2[co][q], c1_padded[ci][y + ky - 1][x + kx - 1]), (y, x) the chosen position of window q;
//   s2b[co] = sum chain of g2[co][q] over the same windows
//   dc1[ci][y][x] = fma chain over (co, ky, kx) ascending, of the taps only whose conv2 output (y - ky + 1, x - kx + 1)
//             lies inside the plane and is the chosen position of a window with c2 > 0, of (g2[co][that window],
//             conv2.w[co][ci][ky][kx]);   g1 = c1 > 0 ? dc1 : +0
//   s1[c][ky][kx] = fma chain over the windows q of channel c in row-major order, those with c1 > 0 only, of
//             (g1[c][q], a_padded[y + ky - 2][x + kx - 2]), a the normalised image as the forward pass computes it,
//             (y, x) the chosen position of window q;   s1b[c] = sum chain of g1[c][q] over the same windows
//   No gradient goes to the image or to the grasp depth.
//  over the batch (k_gq_train_backward_weights, one thread per float of the blob, b ascending from 0 to m-1):
//   out.w[i]     fma chain of (g[b], f2[b][i])                  out.b     sum chain of g[b]
//   fc2.w[o][i]  fma chain of (dz2[b][o], cat[b][i])            fc2.b[o]  sum chain of dz2[b][o]
//   pose.w[j]    fma chain of (dzc[b][F1 + j], u[b])            pose.b[j] sum chain of dzc[b][F1 + j]
//   fc1.w[o][k]  fma chain of (dzc[b][o], c2[b][k])             fc1.b[o]  sum chain of dzc[b][o]
//   conv2.w, conv2.b, conv1.w, conv1.b   sum chains of s2[b], s2b[b], s1[b], s1b[b]
//  d_grad has the blob's layout (K-major conv2 and fc weights), every float of it is written.
//
// ADAM (k_adam_step, one thread per element; omb1 = 1 - beta1 and omb2 = 1 - beta2 once, in float32):
//   m' = rv_fma(beta1, m, omb1 * g);   v' = rv_fma(beta2, v, (omb2 * g) * g)
//   w' = w - (lr * (m' * corr1)) / (fsqrtr(v' * corr2) + eps)
// every product, sum, the square root and the division rounded on its own (correctly: -ffp-contract=off, sqrtf and / as
// rv_cem_refit uses them); corr1 = 1 / (1 - beta1^t) and corr2 = 1 / (1 - beta2^t) come from the caller.
//
// Shapes.  The work is small (about 4 MFLOP per sample backward at the default sizes) and everything is VALU FMA chains but
// the forward pass's MFMA layers: a sample's data gradients and convolution partials in one workgroup of 256 threads with
// c1, the normalised image, g2, g1, the chosen positions and conv2's weights in LDS, and for the gradient at c1 a
// zero-bordered map of four conv2 channels' gradients at a time, so that a tap is one LDS read at a constant offset (about
// 75 KB at the default sizes, dynamic: two workgroups per CU), then one launch over the blob whose threads walk the
// batch; tests/grasp_train_host.py restates all of it in float32 NumPy and the GPU tests compare bit for bit.  Every global
// index is a size_t.
#ifndef RV_DEV_GRASP_TRAIN_H_
#define RV_DEV_GRASP_TRAIN_H_
#include "rv_dev_env.h"
#include "rv_dev_grasp_quality.h"

#define RV_GT_TPB 256

namespace rv {
struct GtArgs {
  const float* images;      // [rows][h][w]
  const float* depths;      // [rows]
  const float* dlogits;     // [rows] (backward)
  float* ws;                // [rows][GtLayout::stride]
  float* logits;            // [rows] (forward)
  float* grad;              // [count] (backward)
  int h, w, c1, c2, f1, f2, p;
  float im_mean, im_inv_std, z_mean, z_inv_std;
  uint32_t rows;
};
// offsets (in floats) into a sample's row of the workspace and into the LDS of k_gq_train_backward_sample
struct GtLayout {
  int N1, c1, i1, c2, i2, cat, f2, u, g, dz2, dzc, s2, s2b, s1, s1b, stride;
  int l_c1, l_img, l_dmap, l_zero, l_g2, l_sel2, l_g1, l_sel1, l_dz2, l_dzc, l_w2, l_floats;
};
__host__ __device__ inline GtLayout gt_layout(int h, int w, int c1, int c2, int f1, int f2, int p) {
  const GqLayout L = gq_layout(h, w, c1, c2, f1, f2, p);
  GtLayout T;
  T.N1 = L.H1 * L.W1;
  T.c1 = 0; T.i1 = T.c1 + c1 * T.N1; T.c2 = T.i1 + c1 * T.N1; T.i2 = T.c2 + L.K1; T.cat = T.i2 + L.K1; T.f2 = T.cat + L.KC;
  T.u = T.f2 + f2; T.g = T.u + 1; T.dz2 = T.g + 1; T.dzc = T.dz2 + f2; T.s2 = T.dzc + L.KC; T.s2b = T.s2 + 9 * c1 * c2;
  T.s1 = T.s2b + c2; T.s1b = T.s1 + 25 * c1; T.stride = T.s1b + c1;
  T.l_c1 = 0; T.l_img = T.l_c1 + c1 * L.PL1; T.l_dmap = T.l_img + L.IH * L.IW + ((L.IH * L.IW) & 1); T.l_zero = T.l_dmap + 8 * L.PL1;
  T.l_g2 = T.l_zero; T.l_sel2 = T.l_g2 + L.K1;
  T.l_g1 = T.l_sel2 + L.K1; T.l_sel1 = T.l_g1 + c1 * T.N1; T.l_dz2 = T.l_sel1 + c1 * T.N1 / 4; T.l_dzc = T.l_dz2 + f2;
  T.l_w2 = T.l_dzc + L.KC; T.l_floats = T.l_w2 + 9 * c1 * c2;
  return T;
}

struct GtAdam { float lr, beta1, beta2, eps, corr1, corr2; };

// gq_pool, and which of the four it took (0 .. 3 = 2 row + column; ties go to the first)
RV_DEV float gt_pool(float v00, float v01, float v10, float v11, float* sel) {
  float m = gq_relu(v00), s = 0.0f;
  const float b = gq_relu(v01), c = gq_relu(v10), d = gq_relu(v11);
  if (b > m) { m = b; s = 1.0f; }
  if (c > m) { m = c; s = 2.0f; }
  if (d > m) { m = d; s = 3.0f; }
  *sel = s;
  return m;
}
// the fma chain from +0 over o ascending of (x[o], w[o]), x in LDS, w a row of the blob in global memory: sixteen loads
// ahead of their sixteen dependent FMAs (one trip to the caches per 16 terms; the order of the chain is not touched)
RV_DEV float gt_dot(const float* x, const float* w, int n) {
  float acc = 0.0f;
  int o = 0;
  for (; o + 16 <= n; o += 16) {
    float wv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wv[i] = w[o + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc = rv_fma(x[o + i], wv[i], acc);
  }
  for (; o < n; ++o) acc = rv_fma(x[o], w[o], acc);
  return acc;
}
}  // namespace rv

// k_grasp_quality (rv_dev_grasp_quality.h) with the workspace stores added: the same chains in the same order
__global__ __launch_bounds__(RV_GQ_TPB, 2) void k_gq_train_forward(rv::GtArgs a, const float* __restrict__ W) {
  using namespace rv;
  extern __shared__ __align__(16) float gq_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = a.h, w = a.w, C1 = a.c1, C2 = a.c2, F1 = a.f1, F2 = a.f2, P = a.p;
  const GqLayout L = gq_layout(h, w, C1, C2, F1, F2, P);
  const GtLayout T = gt_layout(h, w, C1, C2, F1, F2, P);
  float* imgs = gq_lds + L.l_img;
  float* c1s = gq_lds + L.l_c1;
  float* c2s = gq_lds + L.l_c2;
  float* cat = gq_lds + L.l_cat;
  float* f2s = gq_lds + L.l_f2;
  float* w2s = gq_lds + L.l_w2;
  for (int i = tid; i < L.l_w2; i += RV_GQ_TPB) gq_lds[i] = 0.0f;
  for (int i = tid; i < 9 * C1 * C2; i += RV_GQ_TPB) w2s[i] = W[L.c2w + i];
  __syncthreads();
  const size_t row0 = (size_t)blockIdx.x * RV_GQ_BATCH;
  const int nb = (size_t)a.rows - row0 < (size_t)RV_GQ_BATCH ? (int)((size_t)a.rows - row0) : RV_GQ_BATCH;
  const int m16 = lane & 15, kq = lane >> 4;
  int off[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int kl = 4 * j + kq, ci = kl / 9, tap = kl - 9 * ci;
    off[j] = ci * L.PL1 + (tap / 3) * L.RS1 + tap % 3;
  }
  const int W2 = w / 4, tiles = (L.P2 + 3) / 4;

  for (int m = 0; m < nb; ++m) {
    float* wsm = a.ws + (row0 + (size_t)m) * (size_t)T.stride;
    const float* img = a.images + (row0 + (size_t)m) * (size_t)(h * w);
    for (int i = tid; i < h * w; i += RV_GQ_TPB) {
      const int y = i / w, x = i - y * w;
      const float v = img[i] - a.im_mean;
      imgs[(y + 2) * L.IW + x + 2] = v * a.im_inv_std;
    }
    __syncthreads();
    for (int pix = tid; pix < T.N1; pix += RV_GQ_TPB) {
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
        float sel;
        const float pv = gt_pool(v00, v01, v10, v11, &sel);
        c1s[c * L.PL1 + (py + 1) * L.RS1 + px + 1] = pv;
        wsm[(size_t)(T.c1 + c * T.N1 + pix)] = pv;
        wsm[(size_t)(T.i1 + c * T.N1 + pix)] = sel;
      }
    }
    __syncthreads();
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
          const int q = (t0 + 4 * u) * 4 + kq;
          if (nok && q < L.P2) {
            float sel;
            const float pv = gt_pool(acc[u][0], acc[u][1], acc[u][2], acc[u][3], &sel);
            c2m[n * L.P2 + q] = pv;
            wsm[(size_t)(T.c2 + n * L.P2 + q)] = pv;
            wsm[(size_t)(T.i2 + n * L.P2 + q)] = sel;
          }
        }
      }
    }
  }
  __syncthreads();
  gq_fc(c2s, L.S2, W + L.f1w, W + L.f1b, L.K1, F1, cat, L.SC, wave, lane);
  for (int i = tid; i < RV_GQ_BATCH * P; i += RV_GQ_TPB) {
    const int m = i / P, j = i - m * P;
    float v = 0.0f;
    if (m < nb) {
      const float u = (a.depths[row0 + (size_t)m] - a.z_mean) * a.z_inv_std;
      v = gq_relu(rv_fma(u, W[L.pw + j], W[L.pb + j]));
      if (j == 0) a.ws[(row0 + (size_t)m) * (size_t)T.stride + (size_t)T.u] = u;
    }
    cat[m * L.SC + F1 + j] = v;
  }
  __syncthreads();
  for (int i = tid; i < nb * L.KC; i += RV_GQ_TPB) {
    const int m = i / L.KC, j = i - m * L.KC;
    a.ws[(row0 + (size_t)m) * (size_t)T.stride + (size_t)(T.cat + j)] = cat[m * L.SC + j];
  }
  gq_fc(cat, L.SC, W + L.f2w, W + L.f2b, L.KC, F2, f2s, L.SF, wave, lane);
  __syncthreads();
  for (int i = tid; i < nb * F2; i += RV_GQ_TPB) {
    const int m = i / F2, j = i - m * F2;
    a.ws[(row0 + (size_t)m) * (size_t)T.stride + (size_t)(T.f2 + j)] = f2s[m * L.SF + j];
  }
  if (tid < nb) {
    float acc = W[L.ob];
    for (int k = 0; k < F2; ++k) acc = rv_fma(f2s[tid * L.SF + k], W[L.ow + k], acc);
    a.logits[row0 + (size_t)tid] = acc;
  }
}

// the data gradients and the convolutions' partial sums of one sample (the header's "per sample b")
// (two workgroups per CU, as the LDS allows: at most 256 registers)
__global__ __launch_bounds__(RV_GT_TPB, 2) void k_gq_train_backward_sample(rv::GtArgs a, const float* __restrict__ W) {
  using namespace rv;
  extern __shared__ __align__(16) float gt_lds[];
  const int tid = (int)threadIdx.x;
  const int h = a.h, w = a.w, C1 = a.c1, C2 = a.c2, F1 = a.f1, F2 = a.f2, P = a.p;
  const GqLayout L = gq_layout(h, w, C1, C2, F1, F2, P);
  const GtLayout T = gt_layout(h, w, C1, C2, F1, F2, P);
  const size_t b = (size_t)blockIdx.x;
  float* ws = a.ws + b * (size_t)T.stride;
  float* c1p = gt_lds + T.l_c1;
  float* imgs = gt_lds + T.l_img;
  float2* dmap = reinterpret_cast<float2*>(gt_lds + T.l_dmap);      // [4][PL1] {gradient, landed}, 8-byte aligned
  float* g2 = gt_lds + T.l_g2;
  int* sel2 = reinterpret_cast<int*>(gt_lds + T.l_sel2);
  float* g1 = gt_lds + T.l_g1;
  unsigned char* sel1 = reinterpret_cast<unsigned char*>(gt_lds + T.l_sel1);
  float* dz2 = gt_lds + T.l_dz2;
  float* dzc = gt_lds + T.l_dzc;
  float* w2s = gt_lds + T.l_w2;
  const int N1 = T.N1, W1 = L.W1, H1 = L.H1, W2 = w / 4, P2 = L.P2, KC = L.KC, K1 = L.K1;
  for (int i = tid; i < T.l_zero; i += RV_GT_TPB) gt_lds[i] = 0.0f;      // the zero borders of c1 and of the image
  __syncthreads();
  for (int i = tid; i < C1 * N1; i += RV_GT_TPB) {
    const int c = i / N1, r = i - c * N1, y = r / W1, x = r - y * W1;
    c1p[c * L.PL1 + (y + 1) * L.RS1 + x + 1] = ws[T.c1 + i];
    sel1[i] = (unsigned char)((int)ws[T.i1 + i] & 3);
  }
  const float* img = a.images + b * (size_t)(h * w);
  for (int i = tid; i < h * w; i += RV_GT_TPB) {
    const int y = i / w, x = i - y * w;
    const float v = img[i] - a.im_mean;
    imgs[(y + 2) * L.IW + x + 2] = v * a.im_inv_std;
  }
  for (int i = tid; i < 9 * C1 * C2; i += RV_GT_TPB) w2s[i] = W[L.c2w + i];
  const float g = a.dlogits[b];
  if (tid == 0) ws[T.g] = g;
  // -- the head
  for (int i = tid; i < F2; i += RV_GT_TPB) {
    const float t = rv_fma(g, W[L.ow + i], 0.0f);
    const float v = ws[T.f2 + i] > 0.0f ? t : 0.0f;
    dz2[i] = v; ws[T.dz2 + i] = v;
  }
  __syncthreads();
  for (int i = tid; i < KC; i += RV_GT_TPB) {
    const float* wr = W + L.f2w + (size_t)i * (size_t)F2;
    const float acc = gt_dot(dz2, wr, F2);
    const float v = ws[T.cat + i] > 0.0f ? acc : 0.0f;
    dzc[i] = v; ws[T.dzc + i] = v;
  }
  __syncthreads();
  for (int k = tid; k < K1; k += RV_GT_TPB) {
    const float* wr = W + L.f1w + (size_t)k * (size_t)F1;
    const float acc = gt_dot(dzc, wr, F1);
    const bool pass = ws[T.c2 + k] > 0.0f;
    g2[k] = pass ? acc : 0.0f;
    sel2[k] = pass ? ((int)ws[T.i2 + k] & 3) : -1;
  }
  __syncthreads();
  // -- conv2's weights and bias, this sample's part (K-major like the blob: e = (ci 9 + ky 3 + kx) C2 + co)
  for (int e = tid; e < 9 * C1 * C2; e += RV_GT_TPB) {
    const int kk = e / C2, co = e - kk * C2, ci = kk / 9, tap = kk - 9 * ci, ky = tap / 3, kx = tap - 3 * ky;
    const float* src = c1p + ci * L.PL1 + ky * L.RS1 + kx;
    float acc = 0.0f;
#pragma unroll 4
    for (int q = 0; q < P2; ++q) {
      const int s = sel2[co * P2 + q], sp = s & 3;
      const int qy = q / W2, qx = q - qy * W2;
      const float t = rv_fma(g2[co * P2 + q], src[(2 * qy + (sp >> 1)) * L.RS1 + 2 * qx + (sp & 1)], acc);
      acc = s >= 0 ? t : acc;
    }
    ws[T.s2 + e] = acc;
  }
  for (int co = tid; co < C2; co += RV_GT_TPB) {
    float acc = 0.0f;
#pragma unroll 4
    for (int q = 0; q < P2; ++q) {
      const float t = acc + g2[co * P2 + q];
      acc = sel2[co * P2 + q] >= 0 ? t : acc;
    }
    ws[T.s2b + co] = acc;
  }
  // -- the gradient at c1.  Four conv2 channels at a time are spread out into a zero-bordered map of conv2's output plane,
  // {gradient, 1} at the chosen position of a passing window and {0, 0} elsewhere, so that a tap is one 8-byte LDS read at
  // a constant offset from the pixel; co, ky, kx still ascend, and a tap that does not land is still no term
  // (a thread keeps the chains of its pixels in g1 between the groups of four channels: nobody else touches those floats)
  for (int co0 = 0; co0 < C2; co0 += 4) {
    __syncthreads();      // (every wave has left the map of the four channels before, and conv2's partial sums above)
    for (int i = tid; i < 4 * N1; i += RV_GT_TPB) {
      const int cc = i / N1, r = i - cc * N1, yo = r / W1, xo = r - yo * W1;
      const int idx = (co0 + cc) * P2 + (yo >> 1) * W2 + (xo >> 1);
      const bool hit = sel2[idx] == (((yo & 1) << 1) | (xo & 1));
      float2 v;
      v.x = hit ? g2[idx] : 0.0f;
      v.y = hit ? 1.0f : 0.0f;
      dmap[cc * L.PL1 + (yo + 1) * L.RS1 + xo + 1] = v;
    }
    __syncthreads();
    for (int i = tid; i < C1 * N1; i += RV_GT_TPB) {
      const int ci = i / N1, r = i - ci * N1, y = r / W1, x = r - y * W1;
      const float2* dp = dmap + (y + 1) * L.RS1 + x + 1;
      const float* wp = w2s + ci * 9 * C2 + co0;
      float acc = co0 == 0 ? 0.0f : g1[i];
      for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float2 v = dp[cc * L.PL1 + (1 - ky) * L.RS1 + 1 - kx];
            const float t = rv_fma(v.x, wp[(ky * 3 + kx) * C2 + cc], acc);
            acc = v.y != 0.0f ? t : acc;
          }
      if (co0 + 4 >= C2) acc = c1p[ci * L.PL1 + (y + 1) * L.RS1 + x + 1] > 0.0f ? acc : 0.0f;
      g1[i] = acc;
    }
  }
  __syncthreads();
  // -- conv1's weights and bias, this sample's part
  for (int e = tid; e < 25 * C1; e += RV_GT_TPB) {
    const int c = e / 25, tap = e - 25 * c, ky = tap / 5, kx = tap - 5 * ky;
    const float* src = imgs + ky * L.IW + kx;
    float acc = 0.0f;
#pragma unroll 4
    for (int q = 0; q < N1; ++q) {
      const int qy = q / W1, qx = q - qy * W1, sp = sel1[c * N1 + q];
      const float t = rv_fma(g1[c * N1 + q], src[(2 * qy + (sp >> 1)) * L.IW + 2 * qx + (sp & 1)], acc);
      acc = c1p[c * L.PL1 + (qy + 1) * L.RS1 + qx + 1] > 0.0f ? t : acc;
    }
    ws[T.s1 + e] = acc;
  }
  for (int c = tid; c < C1; c += RV_GT_TPB) {
    float acc = 0.0f;
#pragma unroll 4
    for (int q = 0; q < N1; ++q) {
      const int qy = q / W1, qx = q - qy * W1;
      const float t = acc + g1[c * N1 + q];
      acc = c1p[c * L.PL1 + (qy + 1) * L.RS1 + qx + 1] > 0.0f ? t : acc;
    }
    ws[T.s1b + c] = acc;
  }
}

// one thread per float of the blob: its chain over the batch (the header's "over the batch")
__global__ __launch_bounds__(RV_GT_TPB) void k_gq_train_backward_weights(rv::GtArgs a) {
  using namespace rv;
  const GqLayout L = gq_layout(a.h, a.w, a.c1, a.c2, a.f1, a.f2, a.p);
  const GtLayout T = gt_layout(a.h, a.w, a.c1, a.c2, a.f1, a.f2, a.p);
  const size_t e = (size_t)blockIdx.x * RV_GT_TPB + threadIdx.x;
  if (e >= (size_t)L.count) return;
  const long long i = (long long)e;
  // the element is a sum chain of ws[b][oa], or an fma chain of (ws[b][oa], ws[b][ob])
  int oa, ob = -1;
  if (i < L.c1b) oa = T.s1 + (int)(i - L.c1w);
  else if (i < L.c2w) oa = T.s1b + (int)(i - L.c1b);
  else if (i < L.c2b) oa = T.s2 + (int)(i - L.c2w);
  else if (i < L.f1w) oa = T.s2b + (int)(i - L.c2b);
  else if (i < L.f1b) { const int r = (int)(i - L.f1w), k = r / a.f1; oa = T.dzc + (r - k * a.f1); ob = T.c2 + k; }
  else if (i < L.pw) oa = T.dzc + (int)(i - L.f1b);
  else if (i < L.pb) { oa = T.dzc + a.f1 + (int)(i - L.pw); ob = T.u; }
  else if (i < L.f2w) oa = T.dzc + a.f1 + (int)(i - L.pb);
  else if (i < L.f2b) { const int r = (int)(i - L.f2w), k = r / a.f2; oa = T.dz2 + (r - k * a.f2); ob = T.cat + k; }
  else if (i < L.ow) oa = T.dz2 + (int)(i - L.f2b);
  else if (i < L.ob) { oa = T.g; ob = T.f2 + (int)(i - L.ow); }
  else oa = T.g;
  const size_t stride = (size_t)T.stride, rows = (size_t)a.rows;
  const float* pa = a.ws + (size_t)oa;
  float acc = 0.0f;
  if (ob >= 0) {
    const float* pb = a.ws + (size_t)ob;
#pragma unroll 8
    for (size_t b = 0; b < rows; ++b) acc = rv_fma(pa[b * stride], pb[b * stride], acc);
  } else {
#pragma unroll 8
    for (size_t b = 0; b < rows; ++b) acc = acc + pa[b * stride];
  }
  a.grad[e] = acc;
}

__global__ __launch_bounds__(RV_GT_TPB) void k_adam_step(rv::GtAdam p, size_t count, float* w, const float* g, float* m, float* v) {
  using namespace rv;
  const size_t e = (size_t)blockIdx.x * RV_GT_TPB + threadIdx.x;
  if (e >= count) return;
  const float omb1 = 1.0f - p.beta1, omb2 = 1.0f - p.beta2;
  const float ge = g[e];
  const float m1 = rv_fma(p.beta1, m[e], omb1 * ge);
  const float v1 = rv_fma(p.beta2, v[e], (omb2 * ge) * ge);
  const float num = p.lr * (m1 * p.corr1);
  const float den = fsqrtr(v1 * p.corr2) + p.eps;
  m[e] = m1; v[e] = v1;
  w[e] = w[e] - num / den;
}
#endif
