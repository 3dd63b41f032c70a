// rv_dev_ward.h — the second cluster() call of the reference's real-sensor branch on the device (rv_ward_groups; DESIGN.md
// §26).  SegmentedPointCloudObs.get_observation (robovat/observations/camera_obs.py:203-211) runs remove_table ->
// cluster(method='dbscan') -> drops the noise -> cluster() -> group_by_labels; rv_segment_cloud (rv_dev_segment.h) is the
// first three and a grouping of its own, k_ward_groups is the last two: scikit-learn's AgglomerativeClustering(linkage=
// 'ward', n_clusters=C, connectivity = the symmetrised k-nearest-neighbour graph) on the points DBSCAN kept, cut into
// exactly C groups, and the grouping of rv_dev_segment.h's stage 3 on those groups.  One workgroup of RV_WARD_THREADS lanes
// per env.  tests/ward_host.py restates this header in NumPy, operation for operation; the GPU tests compare bit for bit.
//
// Everything in 1 .. 3 is float64, every product and every sum rounded on its own (-ffp-contract=off, no fast-math: `/` is
// IEEE division).  Every choice is the minimum of a tuple that holds ids, so no result depends on the order of a reduction;
// the atomics are integer ORs and counters.
//
// INPUT points: d_labels >= 0 and x - x == 0, y - y == 0, z - z == 0 (all finite), ranked in index order; n = their count.
// A point with a negative label keeps it in d_groups; one with a label >= 0 and a non-finite coordinate gets RV_SEG_INVALID.
// If n > RV_WARD_MAXPTS = 2048, input rank r goes to slot floor(r * RV_WARD_MAXPTS / n) and the first of a slot stays (the
// rule of RV_SEG_MAXPTS): exactly RV_WARD_MAXPTS are kept, the others get RV_SEG_SKIPPED, RV_WARD_FLAG_OVERFLOW is set.
// K = the number of kept points; below, points are named by their kept rank 0 .. K - 1 (index order).
//
// If K <= C: every kept point is its own group (group r = rank r), nothing below 4 runs (COMPONENTS, EDGES_ADDED and
// MERGES are 0), and K < C sets RV_WARD_FLAG_FEWER.  Otherwise:
//
// 1, neighbours (kneighbors_graph(n_neighbors=k, include_self=False)).  k_eff = min(k, K - 1);
//   d2(i, j) = (dx dx + dy dy) + dz dz,  dx = x_i - x_j .. on the coordinates widened to double;
//   N(i) = the k_eff points j != i smallest in (d2(i, j), j);  adj = N u N^T (a symmetric 0/1 matrix, no diagonal).
//   Found per point by one wave: the distances stay in registers, the k_eff-th smallest is bisected on the 64-bit pattern of
//   d2 (monotone for d2 >= 0) with ballots, at most 64 rounds; ties at that value go to the smallest j.
// 2, completion (_fix_connected_components).  The components of adj, numbered by ascending smallest member; for every pair
//   of components a > b the edge (p in a, q in b) that minimises (d2(p, q), p, q) is added, both ways.  COMPONENTS = their
//   number before this, EDGES_ADDED = COMPONENTS (COMPONENTS - 1) / 2.  Components: the union-find of rv_dev_segment.h.
// 3, merging (ward_tree, then _hc_cut).  Cluster r starts with id r, count 1 and sum = its point.  K - C times: among the
//   adjacent live pairs (a, b), id_a > id_b, take the minimum of (w, id_a, id_b),
//     nn = (c_a c_b) / (c_a + c_b),  t_x = sx_a / c_a - sx_b / c_b (likewise y, z),  w = ((t_x t_x + t_y t_y) + t_z t_z) nn
//   (compute_ward_dist; w is the same whichever of the two is called a).  The merged cluster gets id K + step, count c_a +
//   c_b, sum s_a + s_b; its adjacency is the union of both minus the two themselves.  A step that finds no adjacent live
//   pair sets RV_WARD_FLAG_BOUND and ends the loop (never expected: after 2 the graph is connected).  MERGES = the steps
//   taken.  scikit-learn's heap holds every adjacent pair once under that key, pops the smallest whose two clusters are both
//   live, and _hc_cut undoes the last C - 1 merges: the same partition.
//   Here: a cluster lives in a slot (that of its smallest member; the other slot dies), its adjacency is a row of a K x K
//   bit matrix in the caller's workspace, and every live slot caches its best partner (w, slot).  A step takes the minimum
//   of the caches, ORs two rows, lets one lane per neighbour patch its own row and offer itself to the merged cluster, and
//   rescans only the rows of the clusters whose cached partner died (one wave per row).
// 4, numbering.  Groups are numbered by ascending smallest member; d_groups of a kept point = its group's number.  GROUPS =
//   their count (C, or K when K <= C).
// 5, grouping: stage 3 of rv_dev_segment.h with the group as the cluster, float32 copies of the caller's points.  Slot s <
//   GROUPS holds group s with its m members in index order (m >= P: the P members smallest in (key, index), key = o0 of
//   c0 = 0x50000000 | point index;  0 < m < P: draw j takes the member of rank mulhi(o0, m), c0 = 0x60000000 | s << 16 | j);
//   the slots from GROUPS on are empty (count 0, zeros).  c1 = (uint32_t)draw_index, c2 = the GLOBAL env id, c3 =
//   RV_STREAM_PC: the very words of rv_segment_cloud's grouping, on purpose -- this call REPLACES that grouping of the
//   same points for the same draw_index, it does not draw beside it, and where the groups are DBSCAN's clusters (exactly C
//   of them) d_clouds is bit for bit what rv_segment_cloud wrote.
//
// info row: INPUT n, KEPT K, COMPONENTS, EDGES_ADDED, MERGES, GROUPS, 0, FLAGS (RV_WARD_FLAG_*).
// Workspace per env: the bit matrix (RV_WARD_MAXPTS rows of RV_WARD_ROW_WORDS 64-bit words, 512 KiB), then RV_WARD_MAXPTS
// words kept rank -> point index.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_env.h"
#include "rv_dev_segment.h"

namespace rv {

#define RV_WARD_THREADS 1024
#define RV_WARD_WAVES (RV_WARD_THREADS / 64)
#define RV_WARD_PER (RV_WARD_MAXPTS / RV_WARD_THREADS)
#define RV_WARD_ROW_WORDS (RV_WARD_MAXPTS / 64)
#define RV_WARD_NQ (RV_WARD_MAXPTS / 64)
#define RV_WARD_ENV_BYTES ((size_t)RV_WARD_MAXPTS * RV_WARD_ROW_WORDS * 8 + (size_t)RV_WARD_MAXPTS * 4)
#define RV_WARD_NONE 0x7fffffff
static_assert(RV_WARD_THREADS == RV_SEG_THREADS, "seg_scan counts RV_SEG_WAVES waves");
static_assert(RV_WARD_FLAG_BOUND == RV_SEG_FLAG_BOUND, "seg_find and seg_union set the flag here too");
static_assert(RV_WARD_ROW_WORDS == 32, "one lane per half word in ward_scan_row, lanes 0 .. 31 in the row merge");

#if RV_ON_DEVICE
struct WardArgs {
  rv_ward_params p;
  const float* pts; const int32_t* labels;      // [count][M][3], [count][M]
  int M, env_first;
  unsigned long long* adj;                      // workspace: [count][RV_WARD_MAXPTS][RV_WARD_ROW_WORDS]
  int32_t* idx;                                 // workspace: [count][RV_WARD_MAXPTS], kept rank -> point index
  int32_t* groups; float* clouds; int32_t* slot_counts; int32_t* info;
};

// the order of (w, hi, lo); `who` rides along and breaks the tie of one pair seen from both of its slots
RV_DEV bool ward_less(double w1, int h1, int l1, int s1, double w2, int h2, int l2, int s2) {
  if (w1 != w2) return w1 < w2;
  if (h1 != h2) return h1 < h2;
  if (l1 != l2) return l1 < l2;
  return s1 < s2;
}
// the minimum over the wave, in every lane
RV_DEV void ward_wave_min(double& w, int& hi, int& lo, int& who) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w2 = __shfl_xor(w, o);
    const int h2 = __shfl_xor(hi, o), l2 = __shfl_xor(lo, o), s2 = __shfl_xor(who, o);
    if (ward_less(w2, h2, l2, s2, w, hi, lo, who)) { w = w2; hi = h2; lo = l2; who = s2; }
  }
}
RV_DEV double ward_w(const double (*mean)[RV_WARD_MAXPTS], const int* cnt, int a, int b) {
  const double ca = (double)cnt[a], cb = (double)cnt[b];
  const double nn = (ca * cb) / (ca + cb);
  const double tx = mean[0][a] - mean[0][b], ty = mean[1][a] - mean[1][b], tz = mean[2][a] - mean[2][b];
  return ((tx * tx + ty * ty) + tz * tz) * nn;
}
// the best partner of slot t among the set bits of its row, by one wave: (w, hi id, lo id, partner slot) in every lane,
// who = -1 when the row is empty.  Each lane takes 32 bits of the row.
RV_DEV void ward_scan_row(const unsigned long long* row, int t, const double (*mean)[RV_WARD_MAXPTS], const int* cnt, const int* id,
                          double& w, int& hi, int& lo, int& who) {
  const int lane = (int)threadIdx.x & 63;
  uint32_t bits = (uint32_t)(row[lane >> 1] >> (32 * (lane & 1)));
  const int base = 32 * lane, idt = id[t];
  w = __builtin_huge_val(); hi = RV_WARD_NONE; lo = RV_WARD_NONE; who = -1;
  for (int it = 0; it < 32; ++it) {
    if (!bits) break;
    const int j = base + __ffs((int)bits) - 1;
    bits &= bits - 1u;
    const double wj = ward_w(mean, cnt, t, j);
    const int idj = id[j], h = idt > idj ? idt : idj, l = idt > idj ? idj : idt;
    if (ward_less(wj, h, l, j, w, hi, lo, who)) { w = wj; hi = h; lo = l; who = j; }
  }
  ward_wave_min(w, hi, lo, who);
}

__global__ __launch_bounds__(RV_WARD_THREADS) void k_ward_groups(const rv_config* cfg, WardArgs a) {
  // per slot: the mean and the sum of its cluster (at first both are the point), the cached best partner, id, count, and
  // where a dead slot went.  s_bw doubles as the member lists of stages 2 and 5.
  __shared__ double s_mean[3][RV_WARD_MAXPTS];
  __shared__ double s_sum[3][RV_WARD_MAXPTS];
  __shared__ double s_bw[RV_WARD_MAXPTS];
  __shared__ int s_partner[RV_WARD_MAXPTS], s_id[RV_WARD_MAXPTS], s_cnt[RV_WARD_MAXPTS], s_link[RV_WARD_MAXPTS], s_vict[RV_WARD_MAXPTS];
  __shared__ unsigned long long s_row[RV_WARD_ROW_WORDS];
  __shared__ double s_rw[RV_WARD_WAVES];
  __shared__ int s_rh[RV_WARD_WAVES], s_rl[RV_WARD_WAVES], s_rs[RV_WARD_WAVES];
  __shared__ int s_wv[RV_WARD_WAVES];
  __shared__ int s_n, s_nvict, s_flags;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int e = (int)blockIdx.x, M = a.M;
  const uint32_t gid = (uint32_t)(cfg->env_id_offset + a.env_first + e), draw = (uint32_t)a.p.draw_index;
  const float* pts = a.pts + (size_t)e * M * 3;
  const int32_t* labels = a.labels + (size_t)e * M;
  int32_t* groups = a.groups + (size_t)e * M;
  unsigned long long* adj = a.adj + (size_t)e * RV_WARD_MAXPTS * RV_WARD_ROW_WORDS;
  int32_t* idx = a.idx + (size_t)e * RV_WARD_MAXPTS;
  const int C = a.p.num_groups, P = a.p.num_points;
  int fl = 0;
  if (tid == 0) { s_n = 0; s_nvict = 0; s_flags = 0; }
  __syncthreads();

  // ---- the input points, counted; everything else keeps its label
  {
    int c = 0;
    for (int base = 0; base < M; base += RV_WARD_THREADS) {
      const int i = base + tid;
      if (i < M) {
        const int l = labels[i];
        if (l < 0) groups[i] = l;
        else if (seg_finite(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2])) ++c;
        else groups[i] = RV_SEG_INVALID;
      }
    }
    if (c) atomicAdd(&s_n, c);
  }
  __syncthreads();
  const int n = s_n;
  const int K = n < RV_WARD_MAXPTS ? n : RV_WARD_MAXPTS;
  if (n > RV_WARD_MAXPTS) fl |= RV_WARD_FLAG_OVERFLOW;
  if (K < C) fl |= RV_WARD_FLAG_FEWER;

  // ---- ranked, thinned to RV_WARD_MAXPTS, into LDS
  {
    int r_base = 0;
    for (int base = 0; base < M; base += RV_WARD_THREADS) {
      const int i = base + tid;
      bool in = false;
      float x = 0.0f, y = 0.0f, z = 0.0f;
      if (i < M && labels[i] >= 0) {
        x = pts[3 * (size_t)i]; y = pts[3 * (size_t)i + 1]; z = pts[3 * (size_t)i + 2];
        in = seg_finite(x, y, z);
      }
      int tot;
      const int r = r_base + seg_scan(in, s_wv, &tot);
      if (in) {
        int k = r; bool keep = true;
        if (n > RV_WARD_MAXPTS) {
          k = (int)(((uint64_t)r * RV_WARD_MAXPTS) / (uint64_t)n);
          keep = r == 0 || (int)(((uint64_t)(r - 1) * RV_WARD_MAXPTS) / (uint64_t)n) != k;
        }
        if (keep && k < K) {
          s_sum[0][k] = (double)x; s_sum[1][k] = (double)y; s_sum[2][k] = (double)z;
          s_mean[0][k] = (double)x; s_mean[1][k] = (double)y; s_mean[2][k] = (double)z;
          idx[k] = i;
        } else groups[i] = RV_SEG_SKIPPED;
      }
      r_base += tot;
    }
  }
  __syncthreads();

  int lab[RV_WARD_PER];
  int ngroups = K, ncomp = 0, merges = 0;
#pragma unroll
  for (int q = 0; q < RV_WARD_PER; ++q) { const int t = tid + RV_WARD_THREADS * q; lab[q] = t < K ? t : -1; }

  if (K > C) {
    // ---- 1: the neighbour graph.  The rows start empty; s_partner is the union-find's parent array until stage 3
    for (int t = tid; t < K * RV_WARD_ROW_WORDS; t += RV_WARD_THREADS) adj[t] = 0ull;
#pragma unroll
    for (int q = 0; q < RV_WARD_PER; ++q) { const int t = tid + RV_WARD_THREADS * q; if (t < K) s_partner[t] = t; }
    __syncthreads();
    const int nq = (K + 63) >> 6;
    const int keff = a.p.num_neighbors < K - 1 ? a.p.num_neighbors : K - 1;
    for (int i = wv; i < K; i += RV_WARD_WAVES) {
      const double xi = s_sum[0][i], yi = s_sum[1][i], zi = s_sum[2][i];
      unsigned long long b[RV_WARD_NQ];
#pragma unroll
      for (int q = 0; q < RV_WARD_NQ; ++q) {
        const int j = lane + 64 * q;
        b[q] = 0x7ff0000000000000ull;      // (+inf: beyond every distance)
        if (q < nq && j < K && j != i) {
          const double dx = xi - s_sum[0][j], dy = yi - s_sum[1][j], dz = zi - s_sum[2][j];
          b[q] = (unsigned long long)__double_as_longlong((dx * dx + dy * dy) + dz * dz);
        }
      }
      // the smallest T with at least k_eff distances <= T -- or any T with exactly k_eff, which selects the same set
      unsigned long long lo = 0ull, hi = 0x7fefffffffffffffull;
      for (int it = 0; it < 64; ++it) {
        if (lo >= hi) break;
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        int c = 0;
#pragma unroll
        for (int q = 0; q < RV_WARD_NQ; ++q) if (q < nq) c += __popcll(__ballot(b[q] <= mid));
        if (c == keff) { lo = mid; hi = mid; }
        else if (c > keff) hi = mid;
        else lo = mid + 1ull;
      }
      const unsigned long long T = lo;
      int lt = 0;
#pragma unroll
      for (int q = 0; q < RV_WARD_NQ; ++q) if (q < nq) lt += __popcll(__ballot(b[q] < T));
      const int room = keff - lt;
      int ties = 0;
      unsigned long long* row = adj + (size_t)i * RV_WARD_ROW_WORDS;
#pragma unroll
      for (int q = 0; q < RV_WARD_NQ; ++q)
        if (q < nq) {
          const bool tie = b[q] == T;
          const unsigned long long tb = __ballot(tie);
          const int rk = ties + __popcll(tb & ((1ull << lane) - 1ull));
          const bool in = b[q] < T || (tie && rk < room);
          ties += __popcll(tb);
          const unsigned long long mb = __ballot(in);
          if (lane == 0 && mb) atomicOr(&row[q], mb);
          if (in) atomicOr(&adj[(size_t)(lane + 64 * q) * RV_WARD_ROW_WORDS + (i >> 6)], 1ull << (i & 63));
        }
    }
    __syncthreads();

    // ---- 2: components (the union-find of rv_dev_segment.h: the root is the smallest member), then the missing edges
    for (int q = 0; q < RV_WARD_PER; ++q) {
      const int t = tid + RV_WARD_THREADS * q;
      if (t >= K) continue;
      const unsigned long long* row = adj + (size_t)t * RV_WARD_ROW_WORDS;
      for (int wd = 0; wd <= (t >> 6); ++wd) {
        unsigned long long bits = row[wd];
        for (int it = 0; it < 64; ++it) {
          if (!bits) break;
          const int j = 64 * wd + __ffsll((long long)bits) - 1;
          bits &= bits - 1ull;
          if (j < t) seg_union(s_partner, t, j, K, &fl);
        }
      }
    }
    __syncthreads();
    int root[RV_WARD_PER];
#pragma unroll
    for (int q = 0; q < RV_WARD_PER; ++q) {
      const int t = tid + RV_WARD_THREADS * q;
      root[q] = t < K ? seg_find(s_partner, t, K, &fl) : -1;
    }
    __syncthreads();
    for (int q = 0; q < RV_WARD_PER; ++q) {      // (component numbers: the roots in ascending order, into s_cnt[root])
      const int t = tid + RV_WARD_THREADS * q;
      const bool is_root = t < K && root[q] == t;
      int tot;
      const int num = ncomp + seg_scan(is_root, s_wv, &tot);
      if (is_root) s_cnt[t] = num;
      ncomp += tot;
    }
    __syncthreads();
    if (ncomp > 1) {
      // members sorted by component: sizes in s_id, offsets in s_vict, cursors in s_link, the list in s_bw's bytes
      int* s_mem = reinterpret_cast<int*>(s_bw);
      int cn[RV_WARD_PER];
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) { const int t = tid + RV_WARD_THREADS * q; cn[q] = t < K ? s_cnt[root[q]] : -1; if (t < ncomp) s_id[t] = 0; }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) if (cn[q] >= 0) atomicAdd(&s_id[cn[q]], 1);
      __syncthreads();
      if (tid == 0) { int at = 0; for (int c = 0; c < ncomp; ++c) { s_vict[c] = at; s_link[c] = at; at += s_id[c]; } }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) if (cn[q] >= 0) s_mem[atomicAdd(&s_link[cn[q]], 1)] = tid + RV_WARD_THREADS * q;
      __syncthreads();
      for (int ca = 1; ca < ncomp; ++ca) {
        const int na = s_id[ca], oa = s_vict[ca];
        for (int cb = wv; cb < ca; cb += RV_WARD_WAVES) {
          const int nb = s_id[cb], ob = s_vict[cb], total = na * nb;
          double w = __builtin_huge_val(); int bp = RV_WARD_NONE, bq = RV_WARD_NONE, who = 0;
          for (int u = lane; u < total; u += 64) {
            const int p = s_mem[oa + u / nb], q = s_mem[ob + u % nb];
            const double dx = s_sum[0][p] - s_sum[0][q], dy = s_sum[1][p] - s_sum[1][q], dz = s_sum[2][p] - s_sum[2][q];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (ward_less(d2, p, q, 0, w, bp, bq, 0)) { w = d2; bp = p; bq = q; }
          }
          ward_wave_min(w, bp, bq, who);
          if (lane == 0 && bp != RV_WARD_NONE) {
            atomicOr(&adj[(size_t)bp * RV_WARD_ROW_WORDS + (bq >> 6)], 1ull << (bq & 63));
            atomicOr(&adj[(size_t)bq * RV_WARD_ROW_WORDS + (bp >> 6)], 1ull << (bp & 63));
          }
        }
      }
    }
    __syncthreads();

    // ---- 3: merging.  Every slot is a live cluster of one point; the caches from a scan of every row
#pragma unroll
    for (int q = 0; q < RV_WARD_PER; ++q) {
      const int t = tid + RV_WARD_THREADS * q;
      if (t < K) { s_id[t] = t; s_cnt[t] = 1; s_link[t] = t; }
    }
    __syncthreads();
    for (int t = wv; t < K; t += RV_WARD_WAVES) {
      double w; int hi, lo, who;
      ward_scan_row(adj + (size_t)t * RV_WARD_ROW_WORDS, t, s_mean, s_cnt, s_id, w, hi, lo, who);
      if (lane == 0) { s_bw[t] = w; s_partner[t] = who; }
    }
    __syncthreads();
    const int steps = K - C;
    for (int step = 0; step < steps; ++step) {
      // the best cached pair
      double w = __builtin_huge_val(); int hi = RV_WARD_NONE, lo = RV_WARD_NONE, who = -1;
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) {
        const int t = tid + RV_WARD_THREADS * q;
        if (t < K && s_cnt[t] > 0 && s_partner[t] >= 0) {
          const int it = s_id[t], ip = s_id[s_partner[t]], h = it > ip ? it : ip, l = it > ip ? ip : it;
          const double wt = s_bw[t];
          if (ward_less(wt, h, l, t, w, hi, lo, who)) { w = wt; hi = h; lo = l; who = t; }
        }
      }
      ward_wave_min(w, hi, lo, who);
      if (lane == 0) { s_rw[wv] = w; s_rh[wv] = hi; s_rl[wv] = lo; s_rs[wv] = who; }
      __syncthreads();
      w = s_rw[0]; hi = s_rh[0]; lo = s_rl[0]; who = s_rs[0];
#pragma unroll
      for (int k = 1; k < RV_WARD_WAVES; ++k)
        if (ward_less(s_rw[k], s_rh[k], s_rl[k], s_rs[k], w, hi, lo, who)) { w = s_rw[k]; hi = s_rh[k]; lo = s_rl[k]; who = s_rs[k]; }
      if (who < 0) { fl |= RV_WARD_FLAG_BOUND; break; }      // (the same in every lane: all of them leave)
      const int other = s_partner[who];
      const int keep = who < other ? who : other, dead = who < other ? other : who, newid = K + step;
      unsigned long long* rowk = adj + (size_t)keep * RV_WARD_ROW_WORDS;
      // the merged row and the merged cluster
      if (tid < RV_WARD_ROW_WORDS) {
        unsigned long long m = rowk[tid] | adj[(size_t)dead * RV_WARD_ROW_WORDS + tid];
        if ((keep >> 6) == tid) m &= ~(1ull << (keep & 63));
        if ((dead >> 6) == tid) m &= ~(1ull << (dead & 63));
        rowk[tid] = m; s_row[tid] = m;
      }
      if (tid == 64) {
        const int c = s_cnt[keep] + s_cnt[dead];
#pragma unroll
        for (int d = 0; d < 3; ++d) { const double s = s_sum[d][keep] + s_sum[d][dead]; s_sum[d][keep] = s; s_mean[d][keep] = s / (double)c; }
        s_cnt[keep] = c; s_cnt[dead] = 0; s_id[keep] = newid; s_link[dead] = keep; s_nvict = 0;
      }
      __syncthreads();
      // one lane per neighbour: its row, its offer to the merged cluster, its own cache
      w = __builtin_huge_val(); hi = RV_WARD_NONE; lo = RV_WARD_NONE; who = -1;
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) {
        const int t = tid + RV_WARD_THREADS * q;
        if (t < K && ((s_row[t >> 6] >> (t & 63)) & 1ull)) {
          unsigned long long* rt = adj + (size_t)t * RV_WARD_ROW_WORDS;      // (nothing comes back: no round trip to wait for)
          atomicAnd(&rt[dead >> 6], ~(1ull << (dead & 63)));
          atomicOr(&rt[keep >> 6], 1ull << (keep & 63));
          const double wn = ward_w(s_mean, s_cnt, t, keep);
          const int idt = s_id[t];
          if (ward_less(wn, newid, idt, t, w, hi, lo, who)) { w = wn; hi = newid; lo = idt; who = t; }
          const int pt = s_partner[t];
          if (pt == keep || pt == dead) s_vict[atomicAdd(&s_nvict, 1)] = t;
          else if (wn < s_bw[t]) { s_bw[t] = wn; s_partner[t] = keep; }      // (equal w: the older pair has the smaller ids)
        }
      }
      ward_wave_min(w, hi, lo, who);
      if (lane == 0) { s_rw[wv] = w; s_rh[wv] = hi; s_rl[wv] = lo; s_rs[wv] = who; }
      __syncthreads();
      if (tid == 0) {
        w = s_rw[0]; hi = s_rh[0]; lo = s_rl[0]; who = s_rs[0];
        for (int k = 1; k < RV_WARD_WAVES; ++k)
          if (ward_less(s_rw[k], s_rh[k], s_rl[k], s_rs[k], w, hi, lo, who)) { w = s_rw[k]; hi = s_rh[k]; lo = s_rl[k]; who = s_rs[k]; }
        s_bw[keep] = w; s_partner[keep] = who;
      }
      // the clusters whose cached partner is gone: one wave per row
      const int nv = s_nvict;
      for (int v = wv; v < nv; v += RV_WARD_WAVES) {
        const int t = s_vict[v];
        double w2; int h2, l2, p2;
        ward_scan_row(adj + (size_t)t * RV_WARD_ROW_WORDS, t, s_mean, s_cnt, s_id, w2, h2, l2, p2);
        if (lane == 0) { s_bw[t] = w2; s_partner[t] = p2; }
      }
      ++merges;
      __syncthreads();
    }
    __syncthreads();

    // ---- 4: the live slots in ascending order (a slot is its cluster's smallest member) are the groups
    int at[RV_WARD_PER];
#pragma unroll
    for (int q = 0; q < RV_WARD_PER; ++q) {
      int f = tid + RV_WARD_THREADS * q;
      at[q] = -1;
      if (f < K) {
        for (int s = 0; s < K; ++s) { if (s_cnt[f] > 0) break; f = s_link[f]; }
        if (s_cnt[f] > 0) at[q] = f; else fl |= RV_WARD_FLAG_BOUND;
      }
    }
    ngroups = 0;
    for (int q = 0; q < RV_WARD_PER; ++q) {
      const int t = tid + RV_WARD_THREADS * q;
      const bool live = t < K && s_cnt[t] > 0;
      int tot;
      const int num = ngroups + seg_scan(live, s_wv, &tot);
      if (live) s_partner[t] = num;
      ngroups += tot;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RV_WARD_PER; ++q) lab[q] = at[q] >= 0 ? s_partner[at[q]] : -1;
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < RV_WARD_PER; ++q) {
    const int t = tid + RV_WARD_THREADS * q;
    if (t < K) groups[idx[t]] = lab[q];
  }
  if (fl) atomicOr(&s_flags, fl);

  // ---- 5: grouping (stage 3 of rv_dev_segment.h); sizes in s_id, member lists and keys in s_bw's bytes
  int* s_size = s_id;
  int* s_mem = reinterpret_cast<int*>(s_bw);
  uint32_t* s_key = reinterpret_cast<uint32_t*>(s_mem + RV_WARD_MAXPTS);
#pragma unroll
  for (int q = 0; q < RV_WARD_PER; ++q) s_size[tid + RV_WARD_THREADS * q] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RV_WARD_PER; ++q) if (lab[q] >= 0) atomicAdd(&s_size[lab[q]], 1);
  __syncthreads();
  for (int s = 0; s < C; ++s) {
    const int m = s < ngroups ? s_size[s] : 0;
    float* out = a.clouds + ((size_t)e * C + s) * (size_t)P * 3;
    if (tid == 0) a.slot_counts[(size_t)e * C + s] = m;
    if (m == 0) {
      for (int j = tid; j < 3 * P; j += RV_WARD_THREADS) out[j] = 0.0f;
      continue;
    }
    int pos0 = 0;
    for (int q = 0; q < RV_WARD_PER; ++q) {
      const bool mine = lab[q] == s;
      int tot;
      const int pos = pos0 + seg_scan(mine, s_wv, &tot);
      if (mine) s_mem[pos] = tid + RV_WARD_THREADS * q;
      pos0 += tot;
    }
    __syncthreads();
    if (m < P) {
      for (int j = tid; j < P; j += RV_WARD_THREADS) {
        const uint32_t r = seg_mulhi(seg_hash(cfg, gid, draw, RV_SEG_DRAW_CTR | ((uint32_t)s << 16) | (uint32_t)j), (uint32_t)m);
        const size_t i = (size_t)idx[s_mem[r]];
        out[3 * j] = pts[3 * i]; out[3 * j + 1] = pts[3 * i + 1]; out[3 * j + 2] = pts[3 * i + 2];
      }
    } else {
      for (int t = tid; t < m; t += RV_WARD_THREADS) s_key[t] = seg_hash(cfg, gid, draw, RV_SEG_KEY_CTR | (uint32_t)idx[s_mem[t]]);
      __syncthreads();
      // the rank of member t among the (key, position) pairs; positions are in index order
      uint32_t key[RV_WARD_PER]; int rk[RV_WARD_PER];
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) { const int t = tid + RV_WARD_THREADS * q; key[q] = t < m ? s_key[t] : 0u; rk[q] = 0; }
      for (int b = 0; b < m; ++b) {
        const uint32_t kb = s_key[b];
#pragma unroll
        for (int q = 0; q < RV_WARD_PER; ++q) rk[q] += (kb < key[q] || (kb == key[q] && b < tid + RV_WARD_THREADS * q)) ? 1 : 0;
      }
#pragma unroll
      for (int q = 0; q < RV_WARD_PER; ++q) {
        const int t = tid + RV_WARD_THREADS * q;
        if (t < m && rk[q] < P) {
          const size_t i = (size_t)idx[s_mem[t]];
          float* o = out + 3 * (size_t)rk[q];
          o[0] = pts[3 * i]; o[1] = pts[3 * i + 1]; o[2] = pts[3 * i + 2];
        }
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    int32_t* inf = a.info + (size_t)e * RV_WARD_INFO_WORDS;
    inf[0] = n; inf[1] = K; inf[2] = ncomp; inf[3] = ncomp * (ncomp - 1) / 2; inf[4] = merges; inf[5] = ngroups; inf[6] = 0;
    inf[7] = s_flags;
  }
}
#endif  // RV_ON_DEVICE

}  // namespace rv
