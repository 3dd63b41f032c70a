// rv_dev_push_route.h — route-following push proposals: S pushes per env that move body 0, the task's target, one cell
// along the layout's tiles towards the goal (rv_get_route_field / rv_policy_route_multi / rv_plan_propose_route,
// DESIGN.md §19).  No counterpart in the reference.  Everything below is float32, every product and every sum rounded on
// its own (-ffp-contract=off).
//
// THE GRID.  8 x 8 cells; cell i = r * 8 + c has the centre (tile_offset[0] + (float)r * tile_size, tile_offset[1] +
// (float)c * tile_size): one multiply, one add per coordinate.  A tile (a, b) of the config's lists is the cell r = a,
// c = b (the host refuses lists with a tile that is no integer pair of the grid).  WALKABLE: RV_TASK_CROSSING -- the
// region tiles and the goal tiles; RV_TASK_INSERTION -- every cell that is no region tile, and the goal tiles.
// D[i] (uint8): the number of 4-neighbour hops through walkable cells from cell i to the nearest goal cell; 0 on a goal
// cell, RV_PR_NONE = 255 on a cell that is not walkable or from which no goal cell is reached.
//   k_route_field: one wave64, lane i = cell i.  d = 0 on goal cells, 255 elsewhere; a round takes the minimum m of the
//   four neighbours' d (__shfl from i +- 8 and i +- 1, each taken only if that neighbour is in the grid: r < 7, r > 0,
//   c < 7, c > 0 -- lanes 7 and 8 are no neighbours) and sets d = m + 1 on a walkable cell where m != 255 and m + 1 < d.
//   Rounds repeat until the __ballot of "changed" is 0, 63 at most (no path through 64 cells is longer).  No LDS, no
//   atomics.  The field is a function of the rv_config alone and no setter touches the tile fields after rv_create: it is
//   computed at a world's first use and kept, 128 bytes of device memory: D[64], then walkable[64] (0 / 1) -- the
//   proposal kernel needs to tell a walkable cell that reaches no goal from one that is not walkable.
//
// WHAT A WAVE OF k_push_proposals_route READS OF ITS ENV (DevEnv, read only): obs_pos[0 .. nb) of the last observation,
// nb = the number of body_movable bodies (1 standing in for 0) as hp_scene counts it, and whether body 0 is one of them.
// Of the config: cspace_low / cspace_high [0 .. 1] (lo0, hi0, lo1, hi1), translation_x / _y (tx, ty), tile_size,
// tile_offset, the seed and env_id_offset.  Indices as RV_HP_SPREAD (rv_dev_push_sampler.h): env m of the world is copy
// m % copies of the source env gid = (env_id_offset + m) / copies; candidate k of env m is kg = (m % copies) * s + k.
//
// PER WAVE, ONCE.  p = obs_pos[0].xy.
//   cur = the walkable cell with the smallest q = dx * dx + dy * dy, (dx, dy) = centre - p; the lowest index among equals.
//         (A q that is not below +inf, a NaN included, counts as +inf.)  Wave arg-min: six __shfl_xor rounds of fminf,
//         then the lowest set bit of __ballot(walkable and q == the minimum).
//   A   = D[cur] == 0: the centre of cur.  D[cur] == 255: the centre of the goal cell (D == 0) with the smallest q, the
//         lowest index among equals.  Otherwise the centre of the first of (r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)
//         that lies in the grid and has D == D[cur] - 1 (one exists: that is what D[cur] means).
//   v = A - p; dist = fsqrtr(vx * vx + vy * vy); (ux, uy) = dist > 1e-6 ? (vx / dist, vy / dist) : (1, 0).
//
// ONE ATTEMPT, from (jit, back, lat, f):
//   (sn, co) = sincosr(jit); dx = ux * co - uy * sn; dy = ux * sn + uy * co                 the push direction
//   x = fclampr((px - dx * back) - dy * lat, lo0, hi0); y = fclampr((py - dy * back) + dx * lat, lo1, hi1)      the start
//   len = (dist + back) * f; m0 = fclampr(dx * (len / tx), -1, 1); m1 = fclampr(dy * (len / ty), -1, 1)         the motion
//   s0 = fclampr((x - mid0) / half0, -1, 1), half0 = 0.5 * (hi0 - lo0), mid0 = 0.5 * (hi0 + lo0); s1 likewise
//   good = for every b < nb: fsqrtr(ex * ex + ey * ey) > start_margin, (ex, ey) = obs_pos[b] - (x, y) -- hp_attempt's
//          "safe", a NaN distance is not safe.
// The action is (s0, s1, m0, m1), written to each of the G goal steps.
// Attempt a of candidate kg draws jit = u(-angle_jitter, angle_jitter), back = u(back_lo, back_hi), lat = u(-lateral,
// lateral), f = u(length_lo, length_hi) (u = rng_uniform), in that order, from the ONE Philox4x32-10 block with key = the
// world's seed and counter words
//     c0 = (step << 26) | (kg << 16) | a        step < 64, kg < 1024, a < 2^15
//     c1 = the policy's seed (rv_push_route_params.seed)
//     c2 = gid
//     c3 = (RV_STREAM_PUSH_ROUTE << 24) | plan_index      plan_index in [0, 2^24); the ids: rv_dev_math.h
// The first good attempt wins (RV_HP_FOUND); with none in max_attempts, attempt max_attempts - 1 as drawn
// (RV_HP_EXHAUSTED).  With keep_nominal, candidate kg == 0 draws nothing: its one attempt is (0, 0.5 * (back_lo +
// back_hi), 0, 1), FOUND or EXHAUSTED by the same test.  An env whose body 0 is not movable gets the action (0, 0, 0, 0)
// and RV_HP_EXHAUSTED.
// k_push_proposals_route: the launch shape of k_push_proposals_spread -- one wave per (env row, candidate), RV_HP_WAVES
// waves per 256-thread workgroup, 64 attempts per round, the lowest set bit of the ballot wins; no LDS, no atomics, no
// barrier; the env's words are wave-uniform loads.  Rows as in rv_dev_push_sampler.h: r = (m * s + k) * h + t.
// tests/push_route_host.py restates this header in float32 NumPy (its field by a queue BFS); the GPU tests compare bit
// for bit.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"
#include "rv_dev_env.h"
#include "rv_dev_push_sampler.h"

namespace rv {

#define RV_PR_GRID 8
#define RV_PR_CELLS (RV_PR_GRID * RV_PR_GRID)
#define RV_PR_NONE 255
#define RV_PR_FIELD_BYTES (2 * RV_PR_CELLS)      // D[64], walkable[64]

// what an attempt reads besides its four numbers; wave-uniform
struct PrScene {
  const float (*pos)[3];
  float lo0, hi0, lo1, hi1, tx, ty;
  float px, py, ux, uy, dist;
  float start_margin;
  int nb;
};

// one attempt (see above); the action to a[0 .. 3]
RV_DEV bool pr_attempt(const PrScene& sc, float jit, float back, float lat, float f, float (&a)[4]) {
  float sn, co; sincosr(jit, &sn, &co);
  const float dx = sc.ux * co - sc.uy * sn, dy = sc.ux * sn + sc.uy * co;
  const float x = fclampr((sc.px - dx * back) - dy * lat, sc.lo0, sc.hi0);
  const float y = fclampr((sc.py - dy * back) + dx * lat, sc.lo1, sc.hi1);
  const float len = (sc.dist + back) * f;
  const float m0 = fclampr(dx * (len / sc.tx), -1.0f, 1.0f);
  const float m1 = fclampr(dy * (len / sc.ty), -1.0f, 1.0f);
  const float s0 = fclampr((x - 0.5f * (sc.hi0 + sc.lo0)) / (0.5f * (sc.hi0 - sc.lo0)), -1.0f, 1.0f);
  const float s1 = fclampr((y - 0.5f * (sc.hi1 + sc.lo1)) / (0.5f * (sc.hi1 - sc.lo1)), -1.0f, 1.0f);
  int safe = 1;
#pragma unroll
  for (int b = 0; b < RV_MAXB; ++b) {
    if (b < sc.nb) {
      const float ex = sc.pos[b][0] - x, ey = sc.pos[b][1] - y;
      if (!(fsqrtr(ex * ex + ey * ey) > sc.start_margin)) safe = 0;
    }
  }
  a[0] = s0; a[1] = s1; a[2] = m0; a[3] = m1;
  return safe != 0;
}

#if RV_ON_DEVICE
struct PrArgs {
  rv_push_route_params p;
  const uint8_t* field;   // D[64], walkable[64] (k_route_field)
  float* actions;         // rows of [G][4]
  int32_t* status;        // one per row, or null
  int S, h, t;            // candidates per env row; the row of (m, k) is (m * S + k) * h + t
};

// is cell (r, c) on the list?  (the host has checked that every tile is an integer pair of the grid)
RV_DEV int pr_listed(const float (*tiles)[2], int n, int r, int c) {
  int on = 0;
  for (int j = 0; j < n; ++j) on |= (int)tiles[j][0] == r && (int)tiles[j][1] == c;
  return on;
}

__global__ __launch_bounds__(64) void k_route_field(const rv_config* c, uint8_t* field) {
  const int i = (int)threadIdx.x & 63, r = i >> 3, cc = i & 7;
  const int n_region = c->n_region < RV_MAXTILES ? c->n_region : RV_MAXTILES;
  const int n_goal = c->n_goal < RV_MAXTILES ? c->n_goal : RV_MAXTILES;
  const int in_region = pr_listed(c->region, n_region, r, cc), in_goal = pr_listed(c->goal, n_goal, r, cc);
  const int walk = in_goal || (c->task == RV_TASK_CROSSING ? in_region : !in_region);
  int d = in_goal ? 0 : RV_PR_NONE;
  for (int round = 0; round < RV_PR_CELLS - 1; ++round) {
    // (every lane takes part in every shuffle; the index wraps inside the wave and the guard drops what wrapped)
    const int dn = __shfl(d, (i + 8) & 63), up = __shfl(d, (i - 8) & 63), rt = __shfl(d, (i + 1) & 63), lf = __shfl(d, (i - 1) & 63);
    int m = RV_PR_NONE;
    if (r < RV_PR_GRID - 1 && dn < m) m = dn;
    if (r > 0 && up < m) m = up;
    if (cc < RV_PR_GRID - 1 && rt < m) m = rt;
    if (cc > 0 && lf < m) m = lf;
    const bool changed = walk && m != RV_PR_NONE && m + 1 < d;
    if (changed) d = m + 1;
    if (!__ballot(changed)) break;
  }
  field[i] = (uint8_t)d;
  field[RV_PR_CELLS + i] = (uint8_t)walk;
}

// the lowest lane among those of `among` with the smallest q; `among` is not empty (wave-uniform result)
RV_DEV int pr_argmin(float q, bool among) {
  const float key = among && q < __builtin_inff() ? q : __builtin_inff();
  float best = key;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o));
  return (int)__ffsll((long long)__ballot(among && key == best)) - 1;
}

__global__ __launch_bounds__(64 * RV_HP_WAVES) void k_push_proposals_route(const DevEnv* envs, int n, const rv_config* c, PrArgs A) {
  const int lane = (int)threadIdx.x & 63;
  // (wave-uniform by construction; said so to the compiler: the env's words become scalar loads)
  const long long w = (long long)blockIdx.x * RV_HP_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= (long long)n * A.S) return;
  const int m = (int)(w / A.S), k = (int)(w % A.S);
  const DevEnv& e = envs[m];
  const int G = c->num_goal_steps > 0 ? c->num_goal_steps : 1;
  const size_t row = ((size_t)m * A.S + k) * A.h + A.t;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!body_movable(e, 0)) {
    if (lane == 0) hp_write(A, G, row, a, RV_HP_EXHAUSTED);
    return;
  }
  PrScene sc;
  int nb = 0;
#pragma unroll
  for (int b = 0; b < RV_MAXB; ++b) nb += body_movable(e, b);
  sc.nb = nb;      // (body 0 is movable: at least 1)
  sc.pos = e.obs_pos;
  sc.lo0 = c->cspace_low[0]; sc.hi0 = c->cspace_high[0]; sc.lo1 = c->cspace_low[1]; sc.hi1 = c->cspace_high[1];
  sc.tx = c->translation_x; sc.ty = c->translation_y;
  sc.start_margin = A.p.start_margin;
  sc.px = e.obs_pos[0][0]; sc.py = e.obs_pos[0][1];
  const uint32_t copies = (uint32_t)A.p.copies;
  const uint32_t gid = (uint32_t)(c->env_id_offset + m) / copies;
  const uint32_t kg = ((uint32_t)m % copies) * (uint32_t)A.S + (uint32_t)k;

  // the aim: lane = cell
  const float size = c->tile_size, off0 = c->tile_offset[0], off1 = c->tile_offset[1];
  const int d = (int)A.field[lane];
  const bool walk = A.field[RV_PR_CELLS + lane] != 0;
  const float cx = off0 + (float)(lane >> 3) * size, cy = off1 + (float)(lane & 7) * size;
  const float qx = cx - sc.px, qy = cy - sc.py;
  const float q = qx * qx + qy * qy;
  const int cur = pr_argmin(q, walk);
  const int d_cur = __shfl(d, cur);
  int aim = cur;
  if (d_cur == RV_PR_NONE) {
    aim = pr_argmin(q, d == 0);
  } else if (d_cur != 0) {
    const int r = cur >> 3, cc = cur & 7;
    // (every lane takes part in every shuffle; a neighbour outside the grid is dropped by the guard)
    const int dn = __shfl(d, (cur + 8) & 63), up = __shfl(d, (cur - 8) & 63), rt = __shfl(d, (cur + 1) & 63), lf = __shfl(d, (cur - 1) & 63);
    if (r < RV_PR_GRID - 1 && dn == d_cur - 1) aim = cur + 8;
    else if (r > 0 && up == d_cur - 1) aim = cur - 8;
    else if (cc < RV_PR_GRID - 1 && rt == d_cur - 1) aim = cur + 1;
    else if (cc > 0 && lf == d_cur - 1) aim = cur - 1;
  }
  aim = __builtin_amdgcn_readfirstlane(aim);
  const float vx = (off0 + (float)(aim >> 3) * size) - sc.px, vy = (off1 + (float)(aim & 7) * size) - sc.py;
  sc.dist = fsqrtr(vx * vx + vy * vy);
  sc.ux = 1.0f; sc.uy = 0.0f;
  if (sc.dist > 1e-6f) { sc.ux = vx / sc.dist; sc.uy = vy / sc.dist; }

  if (A.p.keep_nominal && kg == 0u) {
    const bool good = pr_attempt(sc, 0.0f, 0.5f * (A.p.back_lo + A.p.back_hi), 0.0f, 1.0f, a);
    if (lane == 0) hp_write(A, G, row, a, good ? RV_HP_FOUND : RV_HP_EXHAUSTED);
    return;
  }
  const uint32_t c0 = ((uint32_t)A.p.step << 26) | (kg << 16);
  const uint32_t c3 = (RV_STREAM_PUSH_ROUTE << 24) | (uint32_t)A.p.plan_index;
  const int budget = A.p.max_attempts;
  int found = -1;
  for (int base_att = 0; base_att < budget; base_att += 64) {
    const int att = base_att + lane;
    bool good = false;
    if (att < budget) {
      Rng g = rng_init(c->seed_lo, c->seed_hi, gid, c3, A.p.seed);
      g.c0 = c0 | (uint32_t)att;
      const float jit = rng_uniform(g, -A.p.angle_jitter, A.p.angle_jitter);
      const float back = rng_uniform(g, A.p.back_lo, A.p.back_hi);
      const float lat = rng_uniform(g, -A.p.lateral, A.p.lateral);
      const float f = rng_uniform(g, A.p.length_lo, A.p.length_hi);
      good = pr_attempt(sc, jit, back, lat, f, a);
    }
    const unsigned long long ballot = __ballot(good);
    if (ballot) { found = base_att + (int)__ffsll((long long)ballot) - 1; break; }
  }
  // the winner, or the last attempt of the budget as drawn (its lane took part in the last round)
  const int writer = found >= 0 ? (found & 63) : ((budget - 1) & 63);
  if (lane == writer) hp_write(A, G, row, a, found >= 0 ? RV_HP_FOUND : RV_HP_EXHAUSTED);
}
#endif  // RV_ON_DEVICE

}  // namespace rv
