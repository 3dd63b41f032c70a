// rv_dev_depth_noise.h — the depth sensor noise model of the reference's perception/depth_utils.py on the device
// (rv_depth_noise): one multiplicative Gamma(k, 1/k) sample per image (gamma_noise) and, with probability
// prob, a coarse grid of N(0, sigma^2) values upsampled x R by Pillow's bicubic resize and added where the image is > 0
// (gaussian_noise).  Two kernels on [N][H][W] buffers: k_depth_noise_draw (the per-image scalars and the grid) and
// k_depth_noise_apply.  Everything below is float32, every product and every sum rounded on its own (-ffp-contract=off).
// logr, normal_pair, fsqrtr: rv_dev_cem.h / rv_dev_math.h.
//
// Keys.  One Philox4x32-10 block (o0 .. o3): key = the world's seed (seed_lo, seed_hi), counter words
//   c0 = q                       the noise grid: block q gives the grid values 4 q .. 4 q + 3 in row-major order of the
//                                [h][w] grid, h = H / R, w = W / R: (z[4q], z[4q+1]) = normal_pair(o0, o1), (z[4q+2],
//                                z[4q+3]) = normal_pair(o2, o3), as cem_normals does; values past h * w are dropped
//   c0 = 0x80000000 | attempt    the per-image scalars, attempt = 0 .. 3
//   c1 = rv_depth_noise_params.seed
//   c2 = global env id (env_id_offset + n)
//   c3 = (RV_STREAM_DEPTH_NOISE << 24) | draw_index      draw_index in [0, 2^24)
// -- a function of nothing else: not of N, not of the image size beyond the grid index, not of the other envs.  c3 cannot
// meet another stream's: the ids are distinct (the table of RV_STREAM_* in rv_dev_math.h).  q < 2^31: a grid block
// never meets a scalar block.
//
// Per-image scalars (dn_scalars), from the scalar blocks:
//   applied = (float)(o3 >> 8) * 2^-24 < prob                of attempt 0 (rng_uniform01's arithmetic)
//   g: gamma_shape == 0: g = 1, nothing more is drawn.  Otherwise (k = gamma_shape >= 1) Marsaglia-Tsang:
//     d = k - 0.333333343 (the float32 next to 1/3);  c = 1 / fsqrtr(9 * d)
//     attempt t = 0 .. 3, block c0 = 0x80000000 | t:
//       x = z0 of normal_pair(o0, o1);   t1 = 1 + c * x;   v = (t1 * t1) * t1;   u = (float)((o2 >> 8) + 1) * 2^-24
//       x2 = x * x;   x4 = x2 * x2
//       accept if v > 0 and ( u < 1 - 0.0331 * x4   or   logr(u) < 0.5 * x2 + d * ((1 - v) + logr(v)) )
//       (the second test is evaluated only when the first fails);  on acceptance g = (d * v) / k
//     after four rejections g = 1 exactly (probability about 1e-8 at k = 1000).
//   logr on v: rv_dev_cem.h documents logr on (0, 1].  Its arithmetic -- the split v = 2^e * m by integer arithmetic on
//   the bits, then the polynomial in m -- holds for every positive normal float32, and this header EXTENDS the
//   documented domain to the range v can take: |x| <= 5.77 and c <= 1 / sqrt(6) give t1 in (-1.36, 3.36); t1 is a float32
//   next to 1, so an accepted v = t1^3 lies in [2^-72, 38] -- normal.  CONTRACT on [2^-72, 64) (tests/test_depth_noise_host.py,
//   against float64): error <= 1 ulp of the true value, or <= 2^-24 absolute for v in [1/2, 2] where |log v| < 0.7.
//
// Noise grid: grid[n][i][j] = sigma * z, written only for envs with applied != 0 and only when sigma > 0 (other entries of
// the buffer are left as they are).
//
// The upsampling up(grid), Pillow's Image.resize(BICUBIC) of a mode-F image (what scipy.misc.imresize(..., interp=
// 'bicubic', mode='F') called), restated in float32.  Separable: the HORIZONTAL pass first, its result rounded to float32,
// then the vertical pass.  For output index xx of an axis with n_in grid cells (dn_taps):
//   center = ((float)xx + 0.5) / (float)R
//   lo = max(0, (int)((center - 2) + 0.5));   hi = min(n_in, (int)((center + 2) + 0.5));   nt = hi - lo   (1 .. 4 taps:
//        4 inside, 2 or 3 at a border; (int) truncates towards zero)
//   tap k = 0 .. nt - 1:  t = |((float)(lo + k) - center) + 0.5|
//        wk = ((1.5 * t - 2.5) * t) * t + 1            for t < 1          (Keys' kernel, a = -0.5, support 2)
//        wk = (((t - 5) * t + 8) * t - 4) * -0.5        for 1 <= t < 2,    0 beyond
//   ww = 0; ww = ww + wk in tap order;   wk = wk / ww                     (normalised by their own sum)
//   value = 0; value = value + in[lo + k] * wk in tap order from 0
// Pillow itself keeps the weights and the running sum in float64; tests/test_depth_noise_host.py bounds the difference.
//
// k_depth_noise_apply, one lane per output pixel (P = 4 neighbouring pixels of a row per lane as one float4 when W is a
// multiple of 4 and the buffers are 16-byte aligned, else P = 1):
//   o = depth * g;   if applied and sigma > 0 and o > 0:  o = o + up(grid)[y][x]
// A workgroup of 256 lanes owns a tile of 32 rows x 16 P columns of one env; a lane owns P pixels of two rows and loads
// them first, so that they are in flight during what follows.  When noise is added the workgroup writes the tile's weights
// (one lane per column, one per row) to LDS, then the horizontal pass for the grid rows the tile's rows touch (at most
// 32 / R + 5 <= 36) to LDS -- the grid itself is read from global memory, the four taps of a value as four loads at once --,
// then every lane takes the vertical pass of its pixels from there.  A value of the horizontal pass is the same number
// whichever tile computes it, so the result does not depend on the tiling.  A lane reads only its own depth pixels
// before it writes them: d_out may be d_in.
// tests/depth_noise_host.py restates this header in float32 NumPy, operation for operation; the GPU tests compare bit for bit.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"
#include "rv_dev_cem.h"

namespace rv {

#define RV_DN_MAX_DRAW_INDEX (1 << 24)
#define RV_DN_MAX_RESCALE 8
#define RV_DN_SCALAR_BLOCK 0x80000000u
#define RV_DN_TILE_ROWS 32
#define RV_DN_TILE_HROWS (RV_DN_TILE_ROWS + 4)

// Keys' cubic, a = -0.5
RV_DEV float dn_keys(float t) {
  t = fabsr(t);
  if (t < 1.0f) return ((1.5f * t - 2.5f) * t) * t + 1.0f;
  if (t < 2.0f) return (((t - 5.0f) * t + 8.0f) * t - 4.0f) * -0.5f;
  return 0.0f;
}

// the taps of output index xx: first grid cell *lo, *nt of them, normalised weights w[0 .. *nt - 1] (the rest 0)
RV_DEV void dn_taps(int xx, int R, int n_in, int* lo, int* nt, float (&w)[4]) {
  const float center = ((float)xx + 0.5f) / (float)R;
  int a = (int)((center - 2.0f) + 0.5f), b = (int)((center + 2.0f) + 0.5f);
  if (a < 0) a = 0;
  if (b > n_in) b = n_in;
  int n = b - a;
  if (n > 4) n = 4;
  float ww = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = k < n ? dn_keys(((float)(a + k) - center) + 0.5f) : 0.0f;
    if (k < n) ww = ww + w[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) w[k] = w[k] / ww;
  *lo = a; *nt = n;
}

RV_DEV void dn_block(uint32_t seed_lo, uint32_t seed_hi, uint32_t gid, const rv_depth_noise_params& p, uint32_t c0,
                     uint32_t* o0, uint32_t* o1, uint32_t* o2, uint32_t* o3) {
  philox(c0, p.seed, gid, (RV_STREAM_DEPTH_NOISE << 24) | (uint32_t)p.draw_index, seed_lo, seed_hi, o0, o1, o2, o3);
}

// the per-image scalars of env gid: the gamma multiplier and the flag
RV_DEV void dn_scalars(uint32_t seed_lo, uint32_t seed_hi, uint32_t gid, const rv_depth_noise_params& p, float* g, int* applied) {
  uint32_t o0, o1, o2, o3;
  dn_block(seed_lo, seed_hi, gid, p, RV_DN_SCALAR_BLOCK, &o0, &o1, &o2, &o3);
  *applied = (float)(o3 >> 8) * 5.9604644775390625e-8f < p.prob ? 1 : 0;
  *g = 1.0f;
  const float k = p.gamma_shape;
  if (k == 0.0f) return;
  const float d = k - 0.333333343f;
  const float c = 1.0f / fsqrtr(9.0f * d);
  for (uint32_t t = 0; t < 4u; ++t) {
    if (t > 0u) dn_block(seed_lo, seed_hi, gid, p, RV_DN_SCALAR_BLOCK | t, &o0, &o1, &o2, &o3);
    float x, z1;
    normal_pair(o0, o1, &x, &z1);
    const float t1 = 1.0f + c * x;
    const float v = (t1 * t1) * t1;
    const float u = (float)((o2 >> 8) + 1u) * 5.9604644775390625e-8f;
    const float x2 = x * x, x4 = x2 * x2;
    if (!(v > 0.0f)) continue;
    if (u < 1.0f - 0.0331f * x4 || logr(u) < 0.5f * x2 + d * ((1.0f - v) + logr(v))) { *g = (d * v) / k; return; }
  }
}

#if RV_ON_DEVICE
struct DnArgs {
  rv_depth_noise_params p;
  const float* in; float* out;     // [N][H][W]
  float* g; uint32_t* flag;        // [N] each: what the apply kernel reads
  float* gamma_out; uint8_t* applied_out;   // [N] or null: the caller's records
  float* grid;                     // [N][h][w]
  int h, w, Q;                     // grid size, Q = ceil(h * w / 4) blocks per env
};

// one lane per (n, q); lane q = 0 also draws the env's scalars
__global__ __launch_bounds__(256) void k_depth_noise_draw(const rv_config* cfg, DnArgs a, long long total) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int q = (int)(t % a.Q), n = (int)(t / a.Q);
  const uint32_t gid = (uint32_t)(cfg->env_id_offset + n);
  const uint32_t slo = cfg->seed_lo, shi = cfg->seed_hi;
  uint32_t o0, o1, o2, o3;
  int applied;
  if (q == 0) {
    float g;
    dn_scalars(slo, shi, gid, a.p, &g, &applied);
    a.g[n] = g; a.flag[n] = (uint32_t)applied;
    if (a.gamma_out) a.gamma_out[n] = g;
    if (a.applied_out) a.applied_out[n] = (uint8_t)applied;
  } else {
    dn_block(slo, shi, gid, a.p, RV_DN_SCALAR_BLOCK, &o0, &o1, &o2, &o3);
    applied = (float)(o3 >> 8) * 5.9604644775390625e-8f < a.p.prob ? 1 : 0;
  }
  if (!applied || !(a.p.sigma > 0.0f)) return;
  float z[4];
  dn_block(slo, shi, gid, a.p, (uint32_t)q, &o0, &o1, &o2, &o3);
  normal_pair(o0, o1, &z[0], &z[1]);
  normal_pair(o2, o3, &z[2], &z[3]);
  const int hw = a.h * a.w;
  float* o = a.grid + (size_t)n * hw;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * q + k < hw) o[4 * q + k] = a.p.sigma * z[k];
}

template <int P>
__global__ __launch_bounds__(256) void k_depth_noise_apply(DnArgs a, int tiles_x, int tiles_y) {
  constexpr int TX = 16 * P, TY = RV_DN_TILE_ROWS;
  __shared__ __attribute__((aligned(16))) float s_h[RV_DN_TILE_HROWS * TX];
  __shared__ __attribute__((aligned(16))) float s_wx[TX * 4];
  __shared__ __attribute__((aligned(16))) float s_wy[TY * 4];
  __shared__ int s_xlo[TX], s_xnt[TX], s_ylo[TY], s_ynt[TY];
  const int tid = (int)threadIdx.x;
  const int bx = (int)(blockIdx.x % (unsigned)tiles_x);
  const unsigned rest = blockIdx.x / (unsigned)tiles_x;
  const int by = (int)(rest % (unsigned)tiles_y), n = (int)(rest / (unsigned)tiles_y);
  const int H = a.p.height, W = a.p.width, R = a.p.rescale_factor;
  const int x0 = bx * TX, y0 = by * TY;
  const float g = a.g[n];
  const bool add = a.flag[n] != 0u && a.p.sigma > 0.0f;      // (the same for the whole workgroup)
  // the lane's own pixels first: their loads are in flight while the workgroup stages the upsampling
  const int tx = tid % 16, ty = tid / 16;
  const int x = x0 + tx * P;
  float d[TY / 16][P];
#pragma unroll
  for (int rr = 0; rr < TY / 16; ++rr) {
    const int y = y0 + ty + 16 * rr;
#pragma unroll
    for (int j = 0; j < P; ++j) d[rr][j] = 0.0f;
    if (x < W && y < H) {
      const size_t at = ((size_t)n * H + y) * W + x;
      if constexpr (P == 4) {
        const float4 v = *reinterpret_cast<const float4*>(a.in + at);
        d[rr][0] = v.x; d[rr][1] = v.y; d[rr][2] = v.z; d[rr][3] = v.w;
      } else {
        d[rr][0] = a.in[at];
      }
    }
  }
  if (add) {
    if (tid < TX) {
      float w[4] = {0.0f, 0.0f, 0.0f, 0.0f}; int lo = 0, nt = 0;
      if (x0 + tid < W) dn_taps(x0 + tid, R, a.w, &lo, &nt, w);
      s_xlo[tid] = lo; s_xnt[tid] = nt;
#pragma unroll
      for (int k = 0; k < 4; ++k) s_wx[tid * 4 + k] = w[k];
    } else if (tid < TX + TY) {
      const int r = tid - TX;
      float w[4] = {0.0f, 0.0f, 0.0f, 0.0f}; int lo = 0, nt = 0;
      if (y0 + r < H) dn_taps(y0 + r, R, a.h, &lo, &nt, w);
      s_ylo[r] = lo; s_ynt[r] = nt;
#pragma unroll
      for (int k = 0; k < 4; ++k) s_wy[r * 4 + k] = w[k];
    }
    __syncthreads();
    // the horizontal pass of grid rows [glo, ghi): what rows y0 .. the tile's last touch
    const int last = (H - y0 < TY ? H - y0 : TY) - 1;
    const int glo = s_ylo[0];
    int rows = s_ylo[last] + s_ynt[last] - glo;
    if (rows > RV_DN_TILE_HROWS) rows = RV_DN_TILE_HROWS;
    const float* grid = a.grid + (size_t)n * a.h * a.w;
    for (int i = tid; i < rows * TX; i += 256) {
      const int xi = i % TX, gi = i / TX;
      if (x0 + xi >= W) continue;
      const float* row = grid + (size_t)(glo + gi) * a.w + s_xlo[xi];
      const int nt = s_xnt[xi];
      float v[4], ss = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = row[k < nt ? k : nt - 1];      // (four loads at once; taps past nt are not summed)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nt) ss = ss + v[k] * s_wx[xi * 4 + k];
      s_h[gi * TX + xi] = ss;
    }
    __syncthreads();
  }
  if (x >= W) return;
#pragma unroll
  for (int rr = 0; rr < TY / 16; ++rr) {
    const int r = ty + 16 * rr, y = y0 + r;
    if (y >= H) continue;
    const size_t at = ((size_t)n * H + y) * W + x;
    float o[P];
#pragma unroll
    for (int j = 0; j < P; ++j) o[j] = d[rr][j] * g;
    if (add) {
      const int hr = s_ylo[r] - s_ylo[0], nt = s_ynt[r];
      float up[P];
#pragma unroll
      for (int j = 0; j < P; ++j) up[j] = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nt) {
          const float wk = s_wy[r * 4 + k];
          const float* hp = s_h + (hr + k) * TX + tx * P;
#pragma unroll
          for (int j = 0; j < P; ++j) up[j] = up[j] + hp[j] * wk;
        }
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (o[j] > 0.0f) o[j] = o[j] + up[j];
    }
    if constexpr (P == 4) {
      *reinterpret_cast<float4*>(a.out + at) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      a.out[at] = o[0];
    }
  }
}
#endif  // RV_ON_DEVICE

}  // namespace rv
