// rv_dev_segment.h — the real-sensor branch of the reference's point-cloud observations on the device (rv_deproject,
// rv_segment_cloud).  SegmentedPointCloudObs.get_observation without a simulator (robovat/observations/
// camera_obs.py:182-211) runs remove_table (a RANSAC plane, 1.5 cm) -> cluster(method='dbscan') (eps 0.02, min_samples
// 50) -> drops the noise -> cluster() -> group_by_labels; PointCloudObs (camera_obs.py:90-124) runs remove_table ->
// downsample.  k_segment_cloud is that chain on one cloud per env, one workgroup of RV_SEG_THREADS lanes per env, in three
// stages.  Everything is float32, every product and every sum rounded on its own (-ffp-contract=off); the counts are
// integers, so no result depends on the order of a reduction.  tests/segment_host.py restates this header in NumPy,
// operation for operation; the GPU tests compare bit for bit.
//
// Keys.  One Philox4x32-10 block (o0 .. o3): key = the world's seed, counter words
//   c0 = 0x40000000 | h                 hypothesis h < T of the plane stage (o0, o1, o2)
//   c0 = 0x50000000 | point index       the sampling key of a point (o0); point index < M <= 2^24
//   c0 = 0x60000000 | slot << 16 | j    draw j < P <= 65536 of a slot with fewer than P members (o0); slot < 16
//   c1 = (uint32_t)draw_index,  c2 = the GLOBAL env id (env_id_offset + env_first + e),  c3 = RV_STREAM_PC (the bare id,
//   as pc_hash of rv_dev_obs.h: this is the point-cloud sampler's second form and takes no stream id of its own).
// The point-cloud sampler's own words (RV_PC_KEY_CTR, RV_PC_DRAW_CTR) have bit 31 set or bits 18 .. 30 clear (b <
// RV_MAXB = 4); the words here have bit 31 clear and bits 28 .. 30 in {4, 5, 6}: they cannot meet.
// mulhi(o, n) = (uint32_t)(((uint64_t)o * n) >> 32).
//
// A point is VALID when d_valid is NULL or its byte is non-zero, and x - x == 0, y - y == 0, z - z == 0 (all finite).
// Valid points are ranked in index order; n = their count.  Invalid points get label RV_SEG_INVALID.
//
// Stage 1, plane.  Hypothesis h: ranks r_k = mulhi(o_k, n), k = 0, 1, 2, points a, b, c of those ranks;
//   u = b - a, v = c - a, nv = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), nn = (nv.x nv.x + nv.y nv.y) + nv.z nv.z.
//   VOID when two ranks coincide or nn < 1e-12f.  Otherwise t2 = (thresh * thresh) * nn and a valid point p is an inlier iff
//   d * d <= t2,  d = (nv.x (p.x - a.x) + nv.y (p.y - a.y)) + nv.z (p.z - a.z)        (no square root, no division).
//   The score is the number of inliers; the best hypothesis has the largest score, ties to the smallest h.  Its inliers
//   get label RV_SEG_PLANE; plane = (nv, -((nv.x a.x + nv.y a.y) + nv.z a.z)).  T == 0, n < 3 or every hypothesis void:
//   nothing is removed, plane = 0, best h = -1, RV_SEG_FLAG_NO_PLANE.
//   Deviation: the reference calls PCL's SACSegmentation (its own generator, 50 iterations and a refit of the coefficients
//   as recalled -- neither is in the reference's tree); here the hypotheses are Philox-keyed and the best one is not refitted.
//
// Stage 2, DBSCAN on the survivors (valid, not on the plane), ranked in index order; s = their count.  They are held in
// LDS: at most RV_SEG_MAXPTS = 8192 (96 KiB).  If s > RV_SEG_MAXPTS, survivor rank r goes to slot floor(r * RV_SEG_MAXPTS /
// s) and the first of a slot stays (the rule of RV_PC_MAXPIX): exactly RV_SEG_MAXPTS are kept, evenly
// spaced; the others get label RV_SEG_SKIPPED and RV_SEG_FLAG_OVERFLOW is set.  min_samples is NOT rescaled then.
//   j is a neighbour of i iff  ((dx dx + dy dy) + dz dz) <= eps * eps,  dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j;
//   i is core iff its neighbour count INCLUDING itself is >= min_samples;
//   clusters = the connected components of the core points under that relation, numbered by ascending smallest member
//   (kept rank, which is index order);  a non-core point with a core neighbour takes the SMALLEST cluster number among its
//   core neighbours;  everything else is noise (-1).
// This is the labelling of scikit-learn's DBSCAN (its depth-first sweep finishes cluster k before it starts k + 1;
// tests/golden/segment_golden.json holds its labels).  Components: a union-find over the core points in LDS, the larger
// root linked under the smaller by compare-and-swap, so that the root of a component is its smallest member whatever the
// order.  Every loop is bounded before it starts: a walk to the root takes at most `kept` steps, a link is retried only
// while a root decreases, at most `kept` times; a bound that runs out sets RV_SEG_FLAG_BOUND and the walk returns where
// it stands.  Three passes over the kept pairs: neighbour counts, links (core i against core j < i), borders.
//
// Stage 3, grouping (group_by_labels / downsample, robovat/perception/point_cloud_utils.py:23-39, 134-157).  The C
// largest clusters (core + border members; ties to the smaller number) fill the slots in ascending cluster number; fewer
// clusters than C: the last slots are empty (label -1, count 0) and RV_SEG_FLAG_FEWER is set.  A slot with m members
// (in index order):
//   m >= P: the P members with the smallest (key, index), in that order;  0 < m < P: draw j takes the member of rank
//   mulhi(o0, m);  m == 0: zeros.
//   Deviation: the reference's second cluster() call (Ward agglomeration on a 100-nearest-neighbour graph, which forces
//   exactly num_bodies groups) is not part of this kernel: it is rv_ward_groups (rv_dev_ward.h), which takes
//   the labels written here and replaces this grouping.  Where DBSCAN finds the bodies apart the two agree up to the order
//   of the slots; where bodies touch, Ward splits the merged blob and this leaves a slot empty (RV_SEG_FLAG_FEWER).
//
// info row: RV_SEG_INFO_* of include/rovat.h.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_env.h"

namespace rv {

#define RV_SEG_THREADS 1024
#define RV_SEG_WAVES (RV_SEG_THREADS / 64)
#define RV_SEG_PER (RV_SEG_MAXPTS / RV_SEG_THREADS)
#define RV_SEG_HYP_CTR  0x40000000u
#define RV_SEG_KEY_CTR  0x50000000u
#define RV_SEG_DRAW_CTR 0x60000000u

RV_DEV uint32_t seg_mulhi(uint32_t o, uint32_t n) { return (uint32_t)(((uint64_t)o * (uint64_t)n) >> 32); }
RV_DEV int seg_finite(float x, float y, float z) { return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f; }
// the plane test of one point against (a, nv, t2)
RV_DEV int seg_inlier(const float* hyp, float x, float y, float z) {
  const float d = (hyp[3] * (x - hyp[0]) + hyp[4] * (y - hyp[1])) + hyp[5] * (z - hyp[2]);
  return d * d <= hyp[6];
}

#if RV_ON_DEVICE
struct SegArgs {
  rv_segment_params p;
  const float* pts; const uint8_t* valid;      // [count][M][3], [count][M] or null
  int M, env_first;
  int32_t* labels; float* clouds; int32_t* slot_labels; int32_t* slot_counts; float* plane; int32_t* info;
  int32_t* idx;                                // scratch [count][M]: rank -> point index
};

// the rank of a set flag among the workgroup's lanes in lane order, and their number (two barriers)
RV_DEV int seg_scan(bool f, int* s_w, int* total) {
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const unsigned long long b = __ballot(f);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[wv] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < RV_SEG_WAVES; ++k) { const int c = s_w[k]; if (k < wv) base += c; tot += c; }
  __syncthreads();
  *total = tot;
  return base + before;
}
// the root of i: at most `bound` steps
RV_DEV int seg_find(const volatile int* par, int i, int bound, int* fl) {
  for (int s = 0; s < bound; ++s) { const int p = par[i]; if (p == i) return i; i = p; }
  if (par[i] != i) *fl |= RV_SEG_FLAG_BOUND;
  return i;
}
// one component of a and b: the larger root goes under the smaller; retried only when the larger root got a parent meanwhile
RV_DEV void seg_union(int* par, int a, int b, int bound, int* fl) {
  for (int t = 0; t < bound; ++t) {
    const int ra = seg_find(par, a, bound, fl), rb = seg_find(par, b, bound, fl);
    if (ra == rb) return;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    if (atomicCAS(&par[hi], hi, lo) == hi) return;
    a = hi; b = lo;
  }
  *fl |= RV_SEG_FLAG_BOUND;
}
RV_DEV uint32_t seg_hash(const rv_config* c, uint32_t gid, uint32_t draw, uint32_t ctr) {
  uint32_t o0, o1, o2, o3;
  philox(ctr, draw, gid, RV_STREAM_PC, c->seed_lo, c->seed_hi, &o0, &o1, &o2, &o3);
  return o0;
}

__global__ __launch_bounds__(RV_SEG_THREADS) void k_segment_cloud(const rv_config* cfg, SegArgs a) {
  // s_pts: the hypotheses of stage 1 ([T][8] floats, then [T] scores), the kept points of stage 2 (x[], y[], z[]), the sizes,
  // member lists and keys of stage 3 -- one after the other
  __shared__ __attribute__((aligned(16))) float s_pts[3 * RV_SEG_MAXPTS];
  __shared__ int s_par[RV_SEG_MAXPTS];
  __shared__ int s_w[RV_SEG_WAVES];
  __shared__ int s_best, s_besth, s_flags, s_noise, s_pick;
  __shared__ int s_chosen[RV_SEG_MAXSLOTS], s_chosen_m[RV_SEG_MAXSLOTS];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int e = (int)blockIdx.x, M = a.M;
  const uint32_t gid = (uint32_t)(cfg->env_id_offset + a.env_first + e), draw = (uint32_t)a.p.draw_index;
  const float* pts = a.pts + (size_t)e * M * 3;
  const uint8_t* valid = a.valid ? a.valid + (size_t)e * M : nullptr;
  int32_t* labels = a.labels + (size_t)e * M;
  int32_t* idx = a.idx + (size_t)e * M;
  const int T = a.p.num_hypotheses, C = a.p.num_clusters, P = a.p.num_points;
  int fl = 0;
  if (tid == 0) { s_best = -1; s_besth = 0x7fffffff; s_flags = 0; s_noise = 0; }

  // ---- the valid points, ranked
  int n = 0;
  for (int base = 0; base < M; base += RV_SEG_THREADS) {
    const int i = base + tid;
    bool ok = false;
    if (i < M) {
      ok = (!valid || valid[i]) && seg_finite(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
      if (!ok) labels[i] = RV_SEG_INVALID;
    }
    int tot;
    const int r = seg_scan(ok, s_w, &tot);
    if (ok) idx[n + r] = i;
    n += tot;
  }
  __syncthreads();

  // ---- stage 1: the plane
  float* s_hyp = s_pts;
  int* s_score = reinterpret_cast<int*>(s_pts + 8 * RV_SEG_MAX_HYPOTHESES);
  bool live = false;
  if (tid < RV_SEG_MAX_HYPOTHESES) { s_score[tid] = 0; s_hyp[tid * 8 + 7] = 0.0f; }
  if (tid < T && n >= 3) {
    uint32_t o0, o1, o2, o3;
    philox(RV_SEG_HYP_CTR | (uint32_t)tid, draw, gid, RV_STREAM_PC, cfg->seed_lo, cfg->seed_hi, &o0, &o1, &o2, &o3);
    const uint32_t r0 = seg_mulhi(o0, (uint32_t)n), r1 = seg_mulhi(o1, (uint32_t)n), r2 = seg_mulhi(o2, (uint32_t)n);
    if (r0 != r1 && r0 != r2 && r1 != r2) {
      const v3 pa = ld3(pts + 3 * (size_t)idx[r0]), pb = ld3(pts + 3 * (size_t)idx[r1]), pc = ld3(pts + 3 * (size_t)idx[r2]);
      const v3 u = sub(pb, pa), v = sub(pc, pa);
      const v3 nv = mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
      const float nn = (nv.x * nv.x + nv.y * nv.y) + nv.z * nv.z;
      if (!(nn < 1e-12f)) {
        live = true;
        float* hp = s_hyp + tid * 8;
        hp[0] = pa.x; hp[1] = pa.y; hp[2] = pa.z; hp[3] = nv.x; hp[4] = nv.y; hp[5] = nv.z;
        hp[6] = (a.p.plane_thresh * a.p.plane_thresh) * nn; hp[7] = 1.0f;
      }
    }
  }
  __syncthreads();
  if (T > 0 && n >= 3) {
    for (int base = 0; base < n; base += RV_SEG_THREADS) {
      if (base + (tid & ~63) >= n) break;      // (the whole wave is past the end)
      const int r = base + tid;
      const bool in = r < n;
      float x = 0.0f, y = 0.0f, z = 0.0f;
      if (in) { const size_t i = (size_t)idx[r]; x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2]; }
      for (int h = 0; h < T; ++h) {
        const float* hp = s_hyp + h * 8;
        if (hp[7] == 0.0f) continue;
        const int c = __popcll(__ballot(in && seg_inlier(hp, x, y, z)));
        if (lane == 0 && c) atomicAdd(&s_score[h], c);
      }
    }
  }
  __syncthreads();
  if (live) atomicMax(&s_best, s_score[tid]);
  __syncthreads();
  if (live && s_score[tid] == s_best) atomicMin(&s_besth, tid);
  __syncthreads();
  const bool has_plane = s_best >= 0;
  const int best_h = has_plane ? s_besth : -1, n_plane = has_plane ? s_best : 0;
  float bh[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (has_plane) for (int k = 0; k < 7; ++k) bh[k] = s_hyp[best_h * 8 + k];
  if (!has_plane) fl |= RV_SEG_FLAG_NO_PLANE;
  __syncthreads();      // (s_pts changes hands)

  // ---- the survivors, thinned to RV_SEG_MAXPTS, into LDS; idx[0 .. K) becomes kept rank -> point index
  float* s_x = s_pts; float* s_y = s_pts + RV_SEG_MAXPTS; float* s_z = s_pts + 2 * RV_SEG_MAXPTS;
  const int ns = n - n_plane;
  const int K = ns < RV_SEG_MAXPTS ? ns : RV_SEG_MAXPTS;
  if (ns > RV_SEG_MAXPTS) fl |= RV_SEG_FLAG_OVERFLOW;
  int sr_base = 0;
  for (int base = 0; base < n; base += RV_SEG_THREADS) {
    const int r = base + tid;
    const bool in = r < n;
    int i = 0; float x = 0.0f, y = 0.0f, z = 0.0f;
    if (in) { i = idx[r]; x = pts[3 * (size_t)i]; y = pts[3 * (size_t)i + 1]; z = pts[3 * (size_t)i + 2]; }
    bool surv = in;
    if (in && has_plane && seg_inlier(bh, x, y, z)) { surv = false; labels[i] = RV_SEG_PLANE; }
    int tot;
    const int sr = sr_base + seg_scan(surv, s_w, &tot);      // (every idx[r] of this round is read before the barrier in here)
    if (surv) {
      int k = sr; bool keep = true;
      if (ns > RV_SEG_MAXPTS) {
        k = (int)(((uint64_t)sr * RV_SEG_MAXPTS) / (uint64_t)ns);
        keep = sr == 0 || (int)(((uint64_t)(sr - 1) * RV_SEG_MAXPTS) / (uint64_t)ns) != k;
      }
      if (keep && k < K) { s_x[k] = x; s_y[k] = y; s_z[k] = z; idx[k] = i; }      // (k <= r: a slot no later round reads)
      else labels[i] = RV_SEG_SKIPPED;
    }
    sr_base += tot;
  }
  __syncthreads();

  // ---- stage 2: DBSCAN.  Lane tid owns the kept ranks tid + RV_SEG_THREADS * q
  const int nq = (K + RV_SEG_THREADS - 1) / RV_SEG_THREADS;
  const float e2 = a.p.eps * a.p.eps;
  float px[RV_SEG_PER], py[RV_SEG_PER], pz[RV_SEG_PER];
  int cnt[RV_SEG_PER];
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    const int k = tid + RV_SEG_THREADS * q;
    const bool in = k < K;
    px[q] = in ? s_x[k] : 0.0f; py[q] = in ? s_y[k] : 0.0f; pz[q] = in ? s_z[k] : 0.0f; cnt[q] = 0;
  }
  for (int j = 0; j < K; ++j) {
    const float xj = s_x[j], yj = s_y[j], zj = s_z[j];
#pragma unroll
    for (int q = 0; q < RV_SEG_PER; ++q)
      if (q < nq) {
        const float dx = px[q] - xj, dy = py[q] - yj, dz = pz[q] - zj;
        cnt[q] += ((dx * dx + dy * dy) + dz * dz) <= e2 ? 1 : 0;
      }
  }
  unsigned core = 0u;
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    const int k = tid + RV_SEG_THREADS * q;
    if (k < K) { if (cnt[q] >= a.p.min_samples) core |= 1u << q; s_par[k] = ((core >> q) & 1u) ? k : -1; }
  }
  __syncthreads();
  // links: core i against core j < i
  {
    const int kmax = (tid | 63) + RV_SEG_THREADS * (nq - 1);      // (the wave's largest rank)
    const int jend = kmax < K ? kmax : K;
    if (__ballot(core != 0u))
      for (int j = 0; j < jend; ++j) {
        const float xj = s_x[j], yj = s_y[j], zj = s_z[j];
#pragma unroll
        for (int q = 0; q < RV_SEG_PER; ++q)
          if (q < nq) {
            const int k = tid + RV_SEG_THREADS * q;
            const float dx = px[q] - xj, dy = py[q] - yj, dz = pz[q] - zj;
            if (((core >> q) & 1u) && j < k && ((dx * dx + dy * dy) + dz * dz) <= e2 && s_par[j] >= 0) seg_union(s_par, k, j, K, &fl);
          }
      }
  }
  __syncthreads();
  int root[RV_SEG_PER];
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    const int k = tid + RV_SEG_THREADS * q;
    root[q] = (k < K && ((core >> q) & 1u)) ? seg_find(s_par, k, K, &fl) : -1;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    const int k = tid + RV_SEG_THREADS * q;
    if (k < K) s_par[k] = root[q];      // (the root of every core point, -1 for the others)
  }
  __syncthreads();
  // borders: the smallest root among the core neighbours
  {
    unsigned open = 0u;
#pragma unroll
    for (int q = 0; q < RV_SEG_PER; ++q) if (tid + RV_SEG_THREADS * q < K && !((core >> q) & 1u)) open |= 1u << q;
    if (__ballot(open != 0u))
      for (int j = 0; j < K; ++j) {
        const int rj = s_par[j];
        if (rj < 0) continue;
        const float xj = s_x[j], yj = s_y[j], zj = s_z[j];
#pragma unroll
        for (int q = 0; q < RV_SEG_PER; ++q)
          if (q < nq) {
            const float dx = px[q] - xj, dy = py[q] - yj, dz = pz[q] - zj;
            if (((open >> q) & 1u) && ((dx * dx + dy * dy) + dz * dz) <= e2 && (root[q] < 0 || rj < root[q])) root[q] = rj;
          }
      }
  }
  // cluster numbers: the roots in ascending order
  int ncl = 0;
  int num[RV_SEG_PER];
  for (int q = 0; q < RV_SEG_PER; ++q) {
    if (q >= nq) break;
    const int k = tid + RV_SEG_THREADS * q;
    const bool is_root = k < K && ((core >> q) & 1u) && root[q] == k;
    int tot;
    num[q] = ncl + seg_scan(is_root, s_w, &tot);
    if (!is_root) num[q] = -1;
    ncl += tot;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q)
    if (q < nq && num[q] >= 0) s_par[tid + RV_SEG_THREADS * q] = -2 - num[q];      // (a root now carries its number)
  __syncthreads();
  int lab[RV_SEG_PER];
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    lab[q] = -1;
    if (q < nq && tid + RV_SEG_THREADS * q < K && root[q] >= 0) lab[q] = -2 - s_par[root[q]];
  }
  __syncthreads();
  int noise = 0;
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) {
    const int k = tid + RV_SEG_THREADS * q;
    if (q < nq && k < K) { s_par[k] = lab[q]; labels[idx[k]] = lab[q]; noise += lab[q] < 0 ? 1 : 0; }
  }
  if (noise) atomicAdd(&s_noise, noise);
  if (fl) atomicOr(&s_flags, fl);
  __syncthreads();      // (s_pts changes hands: the points are read from global memory from here on)

  // ---- stage 3: the C largest clusters, sampled
  int* s_size = reinterpret_cast<int*>(s_pts);
  int* s_mem = s_size + RV_SEG_MAXPTS;
  uint32_t* s_key = reinterpret_cast<uint32_t*>(s_mem + RV_SEG_MAXPTS);
  for (int c = tid; c < ncl; c += RV_SEG_THREADS) s_size[c] = 0;
  if (tid < RV_SEG_MAXSLOTS) { s_chosen[tid] = -1; s_chosen_m[tid] = 0; }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RV_SEG_PER; ++q) if (q < nq && lab[q] >= 0) atomicAdd(&s_size[lab[q]], 1);
  __syncthreads();
  int n_chosen = 0;
  for (int s = 0; s < C && s < ncl; ++s) {
    if (tid == 0) s_pick = 0;
    __syncthreads();
    int best = 0;
    for (int c = tid; c < ncl; c += RV_SEG_THREADS) {
      const int sz = s_size[c];
      if (sz > 0) { const int key = (sz << 13) | (RV_SEG_MAXPTS - 1 - c); if (key > best) best = key; }
    }
    if (best) atomicMax(&s_pick, best);
    __syncthreads();
    if (tid == 0) {
      const int c = RV_SEG_MAXPTS - 1 - (s_pick & (RV_SEG_MAXPTS - 1)), m = s_size[c];
      // (kept in ascending cluster number: an insertion among at most 16)
      int at = s;
      while (at > 0 && s_chosen[at - 1] > c) { s_chosen[at] = s_chosen[at - 1]; s_chosen_m[at] = s_chosen_m[at - 1]; --at; }
      s_chosen[at] = c; s_chosen_m[at] = m;
      s_size[c] = -m;
    }
    ++n_chosen;
    __syncthreads();
  }
  if (n_chosen < C) fl |= RV_SEG_FLAG_FEWER;
  for (int s = 0; s < C; ++s) {
    const int c = s_chosen[s], m = s_chosen_m[s];
    float* out = a.clouds + ((size_t)e * C + s) * (size_t)P * 3;
    if (tid == 0) { a.slot_labels[(size_t)e * C + s] = c; a.slot_counts[(size_t)e * C + s] = m; }
    if (m == 0) {
      for (int j = tid; j < 3 * P; j += RV_SEG_THREADS) out[j] = 0.0f;
      continue;
    }
    int at = 0;
    for (int q = 0; q < nq; ++q) {
      const bool mine = lab[q] == c;
      int tot;
      const int pos = at + seg_scan(mine, s_w, &tot);
      if (mine) s_mem[pos] = tid + RV_SEG_THREADS * q;
      at += tot;
    }
    __syncthreads();
    if (m < P) {
      for (int j = tid; j < P; j += RV_SEG_THREADS) {
        const uint32_t r = seg_mulhi(seg_hash(cfg, gid, draw, RV_SEG_DRAW_CTR | ((uint32_t)s << 16) | (uint32_t)j), (uint32_t)m);
        const size_t i = (size_t)idx[s_mem[r]];
        out[3 * j] = pts[3 * i]; out[3 * j + 1] = pts[3 * i + 1]; out[3 * j + 2] = pts[3 * i + 2];
      }
    } else {
      for (int t = tid; t < m; t += RV_SEG_THREADS) s_key[t] = seg_hash(cfg, gid, draw, RV_SEG_KEY_CTR | (uint32_t)idx[s_mem[t]]);
      __syncthreads();
      // the rank of member t among the (key, position) pairs; positions are in index order
      uint32_t key[RV_SEG_PER]; int rk[RV_SEG_PER];
#pragma unroll
      for (int q = 0; q < RV_SEG_PER; ++q) { const int t = tid + RV_SEG_THREADS * q; key[q] = t < m ? s_key[t] : 0u; rk[q] = 0; }
      const int mq = (m + RV_SEG_THREADS - 1) / RV_SEG_THREADS;
      for (int b = 0; b < m; ++b) {
        const uint32_t kb = s_key[b];
#pragma unroll
        for (int q = 0; q < RV_SEG_PER; ++q)
          if (q < mq) rk[q] += (kb < key[q] || (kb == key[q] && b < tid + RV_SEG_THREADS * q)) ? 1 : 0;
      }
#pragma unroll
      for (int q = 0; q < RV_SEG_PER; ++q) {
        const int t = tid + RV_SEG_THREADS * q;
        if (t < m && rk[q] < P) {
          const size_t i = (size_t)idx[s_mem[t]];
          float* o = out + 3 * (size_t)rk[q];
          o[0] = pts[3 * i]; o[1] = pts[3 * i + 1]; o[2] = pts[3 * i + 2];
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* pl = a.plane + (size_t)e * 4;
    pl[0] = bh[3]; pl[1] = bh[4]; pl[2] = bh[5];
    pl[3] = has_plane ? -((bh[3] * bh[0] + bh[4] * bh[1]) + bh[5] * bh[2]) : 0.0f;
    int32_t* inf = a.info + (size_t)e * RV_SEG_INFO_WORDS;
    inf[RV_SEG_INFO_VALID] = n; inf[RV_SEG_INFO_PLANE] = n_plane; inf[RV_SEG_INFO_SURVIVORS] = ns; inf[RV_SEG_INFO_KEPT] = K;
    inf[RV_SEG_INFO_CLUSTERS] = ncl; inf[RV_SEG_INFO_NOISE] = s_noise; inf[RV_SEG_INFO_BEST_H] = best_h;
    inf[RV_SEG_INFO_FLAGS] = s_flags | fl;
  }
}

// rv_deproject: one lane per pixel of the chunk's envs
__global__ __launch_bounds__(256) void k_deproject(const ObsSnap* snaps, int env_first, size_t total, const float* depth,
                                                   float* pts, uint8_t* valid, const rv_config* c) {
  const int H = c->cam_height, W = c->cam_width;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int e = (int)(t / ((size_t)H * W)); const int px = (int)(t % ((size_t)H * W));
  const int v = px / W, u = px - v * W;
  const ObsSnap* s = &snaps[env_first + e];
  const float z = depth[t];
  const v3 p = deproject(s, cam_position(s), (float)u, (float)v, z);
  pts[3 * t] = p.x; pts[3 * t + 1] = p.y; pts[3 * t + 2] = p.z;
  valid[t] = (uint8_t)((z > 0.0f && crop_ok(c, p)) ? 1 : 0);
}
#endif  // RV_ON_DEVICE

}  // namespace rv
