// rv_collide_probe.hip -- the narrow phase of robovat_amd/csrc/rv_dev_collide.h and the cross-lane primitives of
// rv_dev_wave.h under it, one batch function each (TEST INFRASTRUCTURE ONLY; tests/test_collide_probe.py,
// tests/test_gpu_collide_probe.py).  Nothing under robovat_amd/ includes this file.
//
// Compiled twice, like rv_math_probe.hip: by hipcc for gfx950 with exactly robovat_amd.lib.HIPCC_FLAGS (pointers are
// DEVICE pointers), and by g++ -x c++ -DRV_EMULATE (the same bodies in a serial loop, host pointers).
//
// LAUNCH CONTRACT of every device export
//   * A block is ONE whole wave64: __launch_bounds__(64), blockDim.x == 64.
//   * Each 16-lane group (threadIdx.x >> 4, one DPP row) works one item, so a block holds four items; the lanes of a
//     group run the item redundantly, as the env kernel runs a convex query.  (The row-step, all-reduce and whole-wave
//     exports take one value per lane instead: an item is a wave of 64 values, one block each.)
//   * NO lane returns or diverges before the last cross-lane operation of the kernel.  The DPP steps read the
//     neighbouring lanes of the row with bound_ctrl off, and the result register of the inline-asm maximum is write
//     only: a row with an inactive lane yields garbage.  There is no `if (i >= n) return;` here.  Groups past the last
//     item recompute the last item; only the final stores are predicated (and done by lane 0 of the group).
//   * Hull vertices are staged in LDS before the query, then __syncthreads(): the env kernel reads them from LDS, and
//     the out-of-line epa() reads them through FLAT.  Every hull row holds 16 vertices (48 floats) in memory whatever
//     its count, so the staging loads are in bounds; the code under test reads only indices below the count.
//   * Launch on the null stream, hipGetLastError, hipDeviceSynchronize; the error code is the return value.
//   * Every loop of the code under test is bounded (RV_GJK_MAX_ITERS, RV_EPA_MAX_ITERS); the probe adds none of its own
//     beyond copies of fixed length.
// The caller (tests/probe/build.py) checks what the code under test takes on trust: 1 <= count <= 16, 0 <= cached
// simplex size <= 3, cached indices >= 0, manifold size 0..4, a lane index 0..63.
//
// Every export is int f(int n, [int selectors,] pointers...): n items, returns 0, the hipError_t of the launch, or -1
// where the build has no such function (the cross-lane primitives exist on the device only).
#include "../../robovat_amd/csrc/rv_dev_collide.h"

#ifndef RV_PROBE_HASH
#define RV_PROBE_HASH "unknown"
#endif
// sha256 of rv_dev_math.h, rv_dev_wave.h, rv_dev_collide.h and this file as they were at compile time (build.py)
extern "C" const char* probe_source_hash() { return RV_PROBE_HASH; }
extern "C" int probe_on_device() { return RV_ON_DEVICE; }
extern "C" int probe_devman_words() { return (int)(sizeof(rv::DevMan) / 4); }
extern "C" int probe_gjkcache_words() { return (int)(sizeof(rv::GjkCache) / 4); }

using namespace rv;

#define HULL_FLOATS (3 * RV_MAXV_REG)
#define CP_UNPAREN(...) __VA_ARGS__
#define NOT_AVAILABLE (-1)

#if RV_ON_DEVICE
static int cp_finish() {
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return (int)err;
}
// i = the item of this 16-lane group (clamped: a padded group recomputes the last item), store = this lane writes
#define CPROBE(name, PARAMS, ARGS, ...)                                                                             \
  __global__ __launch_bounds__(64) void k_##name(int n, CP_UNPAREN PARAMS) {                                        \
    const int grp = (int)threadIdx.x >> 4, sl = (int)threadIdx.x & 15;                                              \
    const int slot_ = (int)blockIdx.x * 4 + grp;                                                                    \
    const size_t i = (size_t)(slot_ < n ? slot_ : n - 1);                                                           \
    const bool store = slot_ < n && sl == 0;                                                                        \
    (void)grp; (void)sl;                                                                                            \
    __VA_ARGS__                                                                                                     \
  }                                                                                                                 \
  extern "C" int name(int n, CP_UNPAREN PARAMS) {                                                                   \
    if (n <= 0) return 0;                                                                                           \
    hipLaunchKernelGGL(k_##name, dim3((unsigned)((n + 3) / 4)), dim3(64), 0, 0, n, CP_UNPAREN ARGS);                \
    return cp_finish();                                                                                             \
  }
// the group's hull, from global memory into the block's LDS (lane sl brings vertex sl), and the barrier after it
#define STAGE_HULL(dst, src)                                                                                        \
  __shared__ float dst##_lds[4][HULL_FLOATS];                                                                       \
  for (int k_ = 0; k_ < 3; ++k_) dst##_lds[grp][3 * sl + k_] = (src)[HULL_FLOATS * i + 3 * sl + k_];                \
  const float* dst = dst##_lds[grp];
#define STAGE_SYNC() __syncthreads()
#else
#define CPROBE(name, PARAMS, ARGS, ...)                                                                             \
  extern "C" int name(int n, CP_UNPAREN PARAMS) {                                                                   \
    for (size_t i = 0; i < (size_t)n; ++i) { const bool store = true; __VA_ARGS__ }                                 \
    return 0;                                                                                                       \
  }
#define STAGE_HULL(dst, src) const float* dst = (src) + HULL_FLOATS * i;
#define STAGE_SYNC()
#endif

// ---------------------------------------------------------------------------------------------- cross-lane primitives
// x, o: [n][64] words, one per lane of wave (block) number blockIdx.x
#if RV_ON_DEVICE
RV_DEV uint32_t cp_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
RV_DEV uint32_t cp_bits(int x) { return (uint32_t)x; }
// P: 0 row_ror_f, 1 row_ror_i, 2 row_ror_fmax, 3 row_ror_imin, 4 row_ror_min, 5 row_ror_add, 6 grp_ror_max (steps
// N = 1, 2, 4, 8), 7 grp_bcast<N> (N = 0..15)
template <int P, int N> __global__ __launch_bounds__(64) void k_row_step(const uint32_t* x, uint32_t* o) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t u = x[t];
  const float f = __builtin_bit_cast(float, u);
  const int s = (int)u;
  uint32_t r;
  if constexpr (P == 0) r = cp_bits(row_ror_f<N>(f));
  else if constexpr (P == 1) r = cp_bits(row_ror_i<N>(s));
  else if constexpr (P == 2) r = cp_bits(row_ror_fmax<N>(f));
  else if constexpr (P == 3) r = cp_bits(row_ror_imin<N>(s));
  else if constexpr (P == 4) r = cp_bits(row_ror_min<N>(f));
  else if constexpr (P == 5) r = cp_bits(row_ror_add<N>(f));
  else if constexpr (P == 6) r = cp_bits(grp_ror_max<N>(s));
  else r = cp_bits(grp_bcast<N>(f));
  o[t] = r;
}
// the four-step chains 8, 4, 2, 1 as support_v and the solver use them.  P: 0 fmax, 1 imin, 2 min, 3 add
template <int P> __global__ __launch_bounds__(64) void k_row_allreduce(const uint32_t* x, uint32_t* o) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t u = x[t];
  float f = __builtin_bit_cast(float, u);
  int s = (int)u;
  uint32_t r;
  if constexpr (P == 0) { f = row_ror_fmax<8>(f); f = row_ror_fmax<4>(f); f = row_ror_fmax<2>(f); f = row_ror_fmax<1>(f); r = cp_bits(f); }
  else if constexpr (P == 1) { s = row_ror_imin<8>(s); s = row_ror_imin<4>(s); s = row_ror_imin<2>(s); s = row_ror_imin<1>(s); r = cp_bits(s); }
  else if constexpr (P == 2) { f = row_ror_min<8>(f); f = row_ror_min<4>(f); f = row_ror_min<2>(f); f = row_ror_min<1>(f); r = cp_bits(f); }
  else { f = row_ror_add<8>(f); f = row_ror_add<4>(f); f = row_ror_add<2>(f); f = row_ror_add<1>(f); r = cp_bits(f); }
  o[t] = r;
}
__global__ __launch_bounds__(64) void k_wave_minmax(const float* x, const int* lanes, float* o_min, float* o_max,
                                                    float* o_rdlane, float* o_unif) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  const float f = x[t];
  const int l = uni(lanes[blockIdx.x]) & 63;
  const float mn = wave_min(f), mx = wave_max(f), rd = rdlane(f, l), un = unif(f);
  o_min[t] = mn; o_max[t] = mx; o_rdlane[t] = rd; o_unif[t] = un;
}
#define ROW_CASE(P, N) case (P) * 16 + (N): hipLaunchKernelGGL((k_row_step<P, N>), dim3((unsigned)n), dim3(64), 0, 0, x, o); break;
#define ROW_STEPS(P) ROW_CASE(P, 1) ROW_CASE(P, 2) ROW_CASE(P, 4) ROW_CASE(P, 8)
extern "C" int c_row_step(int n, int prim, int N, const uint32_t* x, uint32_t* o) {
  if (n <= 0) return 0;
  if (prim < 0 || prim > 7 || N < 0 || N > 15) return NOT_AVAILABLE;
  switch (prim * 16 + N) {
    ROW_STEPS(0) ROW_STEPS(1) ROW_STEPS(2) ROW_STEPS(3) ROW_STEPS(4) ROW_STEPS(5) ROW_STEPS(6)
    ROW_CASE(7, 0) ROW_CASE(7, 1) ROW_CASE(7, 2) ROW_CASE(7, 3) ROW_CASE(7, 4) ROW_CASE(7, 5) ROW_CASE(7, 6) ROW_CASE(7, 7)
    ROW_CASE(7, 8) ROW_CASE(7, 9) ROW_CASE(7, 10) ROW_CASE(7, 11) ROW_CASE(7, 12) ROW_CASE(7, 13) ROW_CASE(7, 14) ROW_CASE(7, 15)
    default: return NOT_AVAILABLE;
  }
  return cp_finish();
}
extern "C" int c_row_allreduce(int n, int prim, const uint32_t* x, uint32_t* o) {
  if (n <= 0) return 0;
  switch (prim) {
    case 0: hipLaunchKernelGGL(k_row_allreduce<0>, dim3((unsigned)n), dim3(64), 0, 0, x, o); break;
    case 1: hipLaunchKernelGGL(k_row_allreduce<1>, dim3((unsigned)n), dim3(64), 0, 0, x, o); break;
    case 2: hipLaunchKernelGGL(k_row_allreduce<2>, dim3((unsigned)n), dim3(64), 0, 0, x, o); break;
    case 3: hipLaunchKernelGGL(k_row_allreduce<3>, dim3((unsigned)n), dim3(64), 0, 0, x, o); break;
    default: return NOT_AVAILABLE;
  }
  return cp_finish();
}
extern "C" int c_wave_minmax(int n, const float* x, const int* lanes, float* o_min, float* o_max, float* o_rdlane, float* o_unif) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_wave_minmax, dim3((unsigned)n), dim3(64), 0, 0, x, lanes, o_min, o_max, o_rdlane, o_unif);
  return cp_finish();
}
#else
extern "C" int c_row_step(int, int, int, const uint32_t*, uint32_t*) { return NOT_AVAILABLE; }
extern "C" int c_row_allreduce(int, int, const uint32_t*, uint32_t*) { return NOT_AVAILABLE; }
extern "C" int c_wave_minmax(int, const float*, const int*, float*, float*, float*, float*) { return NOT_AVAILABLE; }
#endif

// ---------------------------------------------------------------------------------------------------------- support_v
// verts [n][48], cnt [n], dir [n][3] -> projection [n], index [n], vertex [n][3], support_proj [n]
CPROBE(c_support_v, (const float* verts, const int* cnt, const float* dir, float* o_proj, int* o_idx, float* o_v, float* o_proj2),
       (verts, cnt, dir, o_proj, o_idx, o_v, o_proj2),
  STAGE_HULL(V, verts)
  STAGE_SYNC();
  const int nv = cnt[i];
  const v3 d = ld3(dir + 3 * i);
  float pj = 0.0f; int idx = -1;
  const v3 v = support_v(V, nv, d, &pj, &idx);
  const float p2 = support_proj(V, nv, d);
  if (store) { o_proj[i] = pj; o_idx[i] = idx; st3(o_v + 3 * i, v); o_proj2[i] = p2; })

// ------------------------------------------------------------------------------------------------ sub-simplex solvers
// p [n][6] -> weights [n][2]
CPROBE(c_closest_segment, (const float* p, float* o_l), (p, o_l),
  float l0, l1;
  closest_segment(ld3(p + 6 * i), ld3(p + 6 * i + 3), &l0, &l1);
  if (store) { o_l[2 * i] = l0; o_l[2 * i + 1] = l1; })
// p [n][9] -> weights [n][3]
CPROBE(c_closest_triangle, (const float* p, float* o_l), (p, o_l),
  float l0, l1, l2;
  closest_triangle(ld3(p + 9 * i), ld3(p + 9 * i + 3), ld3(p + 9 * i + 6), &l0, &l1, &l2);
  if (store) { o_l[3 * i] = l0; o_l[3 * i + 1] = l1; o_l[3 * i + 2] = l2; })
// w [n][12], ns [n] (1..4) -> weights [n][4], "a tetrahedron encloses the origin" [n]
CPROBE(c_simplex_weights, (const float* w, const int* ns, float* o_l, int* o_flag), (w, ns, o_l, o_flag),
  Simplex s;
  for (int k = 0; k < 4; ++k) { s.w[k] = ld3(w + 12 * i + 3 * k); s.a[k] = s.w[k]; s.b[k] = mk(0, 0, 0); s.lam[k] = 0.0f; s.ia[k] = k; s.ib[k] = 0; }
  s.n = ns[i];
  float l[4];
  const int flag = simplex_weights(s, l);
  if (store) { for (int k = 0; k < 4; ++k) o_l[4 * i + k] = l[k]; o_flag[i] = flag; })

// ------------------------------------------------------------------------------------------------------------ gjk_epa
// A, B [n][48], nA, nB [n], guess [n][3], max_dist [n], pair [n], use_gc [n] (0: the call passes gc = nullptr),
// gc_in [n][8] (n, pair, ia[3], ib[3]) -> hit [n], res [n][11] (n3, dist, pa3, pb3, lb_out), gc_out [n][8].
// What the query does not write comes out as 0, an lb_out it never wrote as -1.
CPROBE(c_gjk_epa, (const float* A, const int* nA, const float* B, const int* nB, const float* guess, const float* max_dist,
                   const int* pair, const int* use_gc, const int* gc_in, int* o_hit, float* o_res, int* o_gc),
       (A, nA, B, nB, guess, max_dist, pair, use_gc, gc_in, o_hit, o_res, o_gc),
  STAGE_HULL(VA, A)
  STAGE_HULL(VB, B)
  STAGE_SYNC();
  GjkCache gc;
  gc.n = gc_in[8 * i]; gc.pair = gc_in[8 * i + 1];
  for (int k = 0; k < 3; ++k) { gc.ia[k] = gc_in[8 * i + 2 + k]; gc.ib[k] = gc_in[8 * i + 5 + k]; }
  v3 nn = mk(0, 0, 0), pa = mk(0, 0, 0), pb = mk(0, 0, 0);
  float dist = 0.0f, lb = -1.0f;
  const int hit = gjk_epa(VA, nA[i], VB, nB[i], ld3(guess + 3 * i), max_dist[i], &nn, &dist, &pa, &pb, &lb,
                          use_gc[i] ? &gc : nullptr, pair[i]);
  if (store) {
    o_hit[i] = hit;
    st3(o_res + 11 * i, nn); o_res[11 * i + 3] = dist; st3(o_res + 11 * i + 4, pa); st3(o_res + 11 * i + 7, pb); o_res[11 * i + 10] = lb;
    o_gc[8 * i] = gc.n; o_gc[8 * i + 1] = gc.pair;
    for (int k = 0; k < 3; ++k) { o_gc[8 * i + 2 + k] = gc.ia[k]; o_gc[8 * i + 5 + k] = gc.ib[k]; }
  })

// ------------------------------------------------------------------------------------------------- manifold, tangents
// man_in [n][W] words (W = probe_devman_words()), pt [n][11] (la3, lb3, nrm3, dist, breaking), col [n] -> man_out [n][W]
CPROBE(c_man_add, (const uint32_t* man_in, const float* pt, const int* col, uint32_t* man_out), (man_in, pt, col, man_out),
  const size_t W = sizeof(DevMan) / 4;
  DevMan m;
  __builtin_memcpy(&m, man_in + W * i, sizeof(DevMan));
  const float* q = pt + 11 * i;
  man_add(m, ld3(q), ld3(q + 3), ld3(q + 6), q[9], col[i], q[10]);
  if (store) __builtin_memcpy(man_out + W * i, &m, sizeof(DevMan));)
// nrm [n][3] -> t1, t2 [n][6]
CPROBE(c_plane_space, (const float* nrm, float* o_t), (nrm, o_t),
  v3 t1, t2;
  plane_space(ld3(nrm + 3 * i), &t1, &t2);
  if (store) { st3(o_t + 6 * i, t1); st3(o_t + 6 * i + 3, t2); })
