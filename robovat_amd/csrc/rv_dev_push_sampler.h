// rv_dev_push_sampler.h — S aimed pushes per env: the reference's HeuristicPushSampler.sample(..., num_samples = S)
// (heuristic_push_sampler.py:52-123) as a batch primitive, and a planning form of it with keys of its own
// (rv_policy_heuristic_multi / rv_plan_propose).  Everything below is float32, every product and every sum
// rounded on its own (-ffp-contract=off).
//
// What is read of an env (DevEnv, read only): nb = the number of body_movable bodies, 1 standing in for 0; the positions
// obs_pos[0 .. nb) and the counters n_ep = obs_num_episodes, n_st = obs_num_steps of its LAST OBSERVATION -- as
// k_policy_heuristic reads them.  Of the config: cspace_low / cspace_high [0 .. 1] (lo0, hi0, lo1, hi1), translation_x,
// translation_y, the seed and env_id_offset.  An env whose episode is over gets its proposals like any other.
//
// ONE ATTEMPT, from a stream g of uniforms and a target body T -- k_policy_heuristic's lane body (rv_kernels.hip),
// written out again with the margins as parameters (u(lo, hi) = rng_uniform = lo + (hi - lo) * u01, two roundings):
//   s0 = u(-1, 1); s1 = u(-1, 1)                                          the start, normalised
//   ang = EPISODE: base + u(-pi/4, pi/4)      SPREAD: u(-pi, pi)
//   (sn, co) = sincosr(ang)                                               |ang| < 8: within 2 ulp of the true value
//   m0 = fclampr(co + u(-0.3, 0.3), -1, 1); m1 = fclampr(sn + u(-0.3, 0.3), -1, 1)      the motion
//   x = s0 * (0.5 * (hi0 - lo0)) + 0.5 * (hi0 + lo0); y likewise with s1, lo1, hi1       the start, world
//   ex = fclampr(x + m0 * translation_x, lo0, hi0); ey = fclampr(y + m1 * translation_y, lo1, hi1)     the end
//   safe      = for every b < nb:  fsqrtr(dx * dx + dy * dy) > start_margin,   (dx, dy) = obs_pos[b] - (x, y)
//   effective = not (d1 >= motion_margin and d2 >= motion_margin), d1 / d2 the same distance of obs_pos[T] from (x, y) and
//               from (ex, ey)
//   good = safe and effective.  Five uniforms, in that order: two Philox blocks, the second used for one word.
//   A NaN distance is neither safe nor "clear": as in k_policy_heuristic.
// The action of a candidate is (s0, s1, m0, m1), written to each of the G goal steps.
//
// RV_HP_EPISODE -- the reference's sample(position, body_mask, num_episodes, num_steps, num_samples = S).
//   T = n_ep % nb;  base = (float)n_ep * 42, then base - (2 * RV_PI) * ffloorr(base / (2 * RV_PI)).
//   The stream of attempt a is k_policy_heuristic's: rng_init(world seed, global env id, RV_STREAM_HEUR, n_ep * 64 + n_st)
//   with c0 = 2 * a -- ONE sequence of attempts a = 0, 1, 2, ... per env, which the S candidates share as the S calls of
//   the reference's loop share np.random: candidate 0 starts at attempt 0, candidate k at the attempt after the one where
//   candidate k - 1 stopped.  A candidate scans at most max_attempts attempts and takes the first good one (status
//   RV_HP_FOUND); if none is, it takes the LAST attempt of its budget as drawn (RV_HP_EXHAUSTED), as _sample returns it,
//   and the next candidate starts after that one.  Candidate 0 is rv_policy_heuristic bit for bit.
//   a < S * max_attempts <= 2^25, so 2 * a + 1 fits the counter word.
//   k_push_proposals_episode: one wave per env, 64 attempts per round, then __ballot; a wave-uniform loop hands the set
//   bits out in attempt order.  The state of that loop -- round base, position in the round, candidate, budget left --
//   is wave-uniform; the lane of the chosen attempt writes it.
//
// RV_HP_SPREAD -- the planning form (no counterpart in the reference).
//   Env m of the world that is read is copy (m % copies) of the SOURCE env with global id gid = (env_id_offset + m) /
//   copies (copies >= 1; the world of S branches rv_branch fills has copies = S and env_id_offset = S x the source's).
//   Candidate k of env m has the global candidate index kg = (m % copies) * s + k < 1024, aims at T = kg % nb, draws its
//   angle from u(-pi, pi), and has an attempt stream and a budget of max_attempts of its own: attempt a draws from the
//   two Philox4x32-10 blocks with key = the world's seed and counter words
//     c0 = (step << 26) | (kg << 16) | (2 * a + block)      step < 64, kg < 1024, a < 2^15, block in {0, 1}
//     c1 = the policy's seed (rv_push_proposal_params.seed)
//     c2 = gid
//     c3 = (RV_STREAM_PUSH_PROPOSAL << 24) | plan_index      plan_index in [0, 2^24)
//   -- a function of nothing else: not of N, s, copies or of the other envs.  c3 cannot meet another stream's: the ids are
//   distinct (the table of RV_STREAM_* in rv_dev_math.h).
//   Hence s candidates of a source world (copies = 1) and one candidate of each of its s branches (s = 1, copies = s)
//   are the same bits as long as the observations are: what lets step t of a candidate plan be drawn from that branch's
//   own simulated state (rv_plan_propose, step = t).
//   The first good attempt wins (RV_HP_FOUND); with none in the budget, attempt max_attempts - 1 as drawn
//   (RV_HP_EXHAUSTED).
//   k_push_proposals_spread: one wave per (env row, candidate), 64 attempts per round, the lowest set bit of the ballot
//   wins; no LDS, no atomics, no barrier; the env's positions and counters are wave-uniform loads.  RV_HP_WAVES = 4 such
//   waves share a 256-thread workgroup: they never meet (no barrier, no LDS), so packing costs nothing, a workgroup puts
//   one wave on each SIMD of its CU, eight workgroups fill the CU's 32 wave slots (21 VGPRs, no LDS: neither limits),
//   and the dispatcher hands out a quarter of the workgroups that one-wave workgroups would need for the same waves.
//   (That 64-thread workgroups would leave wave slots idle is not claimed: the choice rests on the dispatch count, and
//   neither shape's time has been measured against the other.)
//
// Output row of (env m, candidate k): r = (m * s + k) * h + t -- rv_policy_heuristic_multi has h = 1, t = 0 and writes
// d_actions [M][s][G][4], d_status [M][s]; rv_plan_propose has s = 1 per branch env and writes slice t of
// d_actions [N][S][h][G][4] = [M][h][G][4], d_status [M][h].
// tests/push_proposals_host.py restates this header in float32 NumPy, operation for operation; the GPU tests compare
// bit for bit.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"
#include "rv_dev_env.h"

namespace rv {

#define RV_HP_WAVES 4
#define RV_HP_MAX_STEP 64
#define RV_HP_MAX_PLAN_INDEX (1 << 24)

// what an attempt reads besides its stream; wave-uniform.  The positions stay where they are (DevEnv::obs_pos, read with
// constant indices: scalar loads): a register array of them would be indexed by the target at run time
struct HpScene {
  const float (*pos)[3];
  float lo0, hi0, lo1, hi1, tx, ty;
  float start_margin, motion_margin;
  int nb;
};

// one attempt (see above): draws five uniforms from g, aims at (bx, by) = obs_pos[T]; the action to a[0 .. 3]
RV_DEV bool hp_attempt(Rng& g, const HpScene& sc, bool spread, float base, float bx, float by, float (&a)[4]) {
  const float s0 = rng_uniform(g, -1.0f, 1.0f), s1 = rng_uniform(g, -1.0f, 1.0f);
  const float ang = spread ? rng_uniform(g, -RV_PI, RV_PI) : base + rng_uniform(g, -0.25f * RV_PI, 0.25f * RV_PI);
  float sn, co; sincosr(ang, &sn, &co);
  const float m0 = fclampr(co + rng_uniform(g, -0.3f, 0.3f), -1.0f, 1.0f);
  const float m1 = fclampr(sn + rng_uniform(g, -0.3f, 0.3f), -1.0f, 1.0f);
  const float x = s0 * (0.5f * (sc.hi0 - sc.lo0)) + 0.5f * (sc.hi0 + sc.lo0);
  const float y = s1 * (0.5f * (sc.hi1 - sc.lo1)) + 0.5f * (sc.hi1 + sc.lo1);
  const float ex = fclampr(x + m0 * sc.tx, sc.lo0, sc.hi0);
  const float ey = fclampr(y + m1 * sc.ty, sc.lo1, sc.hi1);
  int safe = 1;
#pragma unroll
  for (int b = 0; b < RV_MAXB; ++b) {
    if (b < sc.nb) {
      const float dx = sc.pos[b][0] - x, dy = sc.pos[b][1] - y;
      if (!(fsqrtr(dx * dx + dy * dy) > sc.start_margin)) safe = 0;
    }
  }
  const float dx1 = bx - x, dy1 = by - y, dx2 = bx - ex, dy2 = by - ey;
  const int clear = fsqrtr(dx1 * dx1 + dy1 * dy1) >= sc.motion_margin && fsqrtr(dx2 * dx2 + dy2 * dy2) >= sc.motion_margin;
  a[0] = s0; a[1] = s1; a[2] = m0; a[3] = m1;
  return safe && !clear;
}

#if RV_ON_DEVICE
struct HpArgs {
  rv_push_proposal_params p;
  float* actions;       // rows of [G][4]
  int32_t* status;      // one per row, or null
  int S, h, t;          // candidates per env row; the row of (m, k) is (m * S + k) * h + t
};

RV_DEV HpScene hp_scene(const DevEnv& e, const rv_config* c, const rv_push_proposal_params& p) {
  HpScene sc;
  int nb = 0;
#pragma unroll
  for (int b = 0; b < RV_MAXB; ++b) nb += body_movable(e, b);
  sc.nb = nb == 0 ? 1 : nb;
  sc.pos = e.obs_pos;
  sc.lo0 = c->cspace_low[0]; sc.hi0 = c->cspace_high[0]; sc.lo1 = c->cspace_low[1]; sc.hi1 = c->cspace_high[1];
  sc.tx = c->translation_x; sc.ty = c->translation_y;
  sc.start_margin = p.start_margin; sc.motion_margin = p.motion_margin;
  return sc;
}
// (Args: HpArgs, or the PrArgs of rv_dev_push_route.h -- the same row layout)
template <class Args>
RV_DEV void hp_write(const Args& A, int G, size_t row, const float (&a)[4], int status) {
  for (int g2 = 0; g2 < G; ++g2) {
    float* o = A.actions + (row * (size_t)G + (size_t)g2) * 4;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
  }
  if (A.status) A.status[row] = status;
}

__global__ __launch_bounds__(64) void k_push_proposals_episode(const DevEnv* envs, int n, const rv_config* c, HpArgs A) {
  const int m = (int)blockIdx.x; if (m >= n) return;
  const int lane = (int)threadIdx.x;
  const DevEnv& e = envs[m];
  const int G = c->num_goal_steps > 0 ? c->num_goal_steps : 1;
  const HpScene sc = hp_scene(e, c, A.p);
  const int n_ep = e.obs_num_episodes, n_st = e.obs_num_steps;
  const int T = n_ep % sc.nb;
  const float bx = sc.pos[T][0], by = sc.pos[T][1];
  float base = (float)n_ep * 42.0f;
  base = base - 2.0f * RV_PI * ffloorr(base / (2.0f * RV_PI));
  const int S = A.S, budget = A.p.max_attempts;
  int k = 0, left = budget;
  for (uint32_t round = 0; k < S; round += 64u) {
    Rng g = rng_init(c->seed_lo, c->seed_hi, (uint32_t)(c->env_id_offset + m), RV_STREAM_HEUR, (uint32_t)(n_ep * 64 + n_st));
    g.c0 = (round + (uint32_t)lane) * 2u;
    float a[4];
    const bool good = hp_attempt(g, sc, false, base, bx, by, a);
    const unsigned long long ballot = __ballot(good);
    // the candidates this round serves, in attempt order: candidate k scans the bits [pos, min(64, pos + left))
    int pos = 0;
    while (k < S && pos < 64) {
      const int end = pos + left < 64 ? pos + left : 64;
      const unsigned long long upto = end == 64 ? ~0ull : ((1ull << end) - 1ull);
      const unsigned long long bits = ballot & upto & ~((1ull << pos) - 1ull);
      if (bits) {                                // found: the next candidate starts behind it
        const int j = (int)__ffsll((long long)bits) - 1;
        if (lane == j) hp_write(A, G, ((size_t)m * S + k) * A.h + A.t, a, RV_HP_FOUND);
        ++k; pos = j + 1; left = budget;
      } else if (pos + left <= 64) {             // the budget ends in this round: its last attempt as drawn
        if (lane == end - 1) hp_write(A, G, ((size_t)m * S + k) * A.h + A.t, a, RV_HP_EXHAUSTED);
        ++k; pos = end; left = budget;
      } else {                                   // the round is used up
        left -= 64 - pos; pos = 64;
      }
    }
  }
}

__global__ __launch_bounds__(64 * RV_HP_WAVES) void k_push_proposals_spread(const DevEnv* envs, int n, const rv_config* c, HpArgs A) {
  const int lane = (int)threadIdx.x & 63;
  // (wave-uniform by construction; said so to the compiler: the env's words become scalar loads)
  const long long w = (long long)blockIdx.x * RV_HP_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= (long long)n * A.S) return;
  const int m = (int)(w / A.S), k = (int)(w % A.S);
  const DevEnv& e = envs[m];
  const int G = c->num_goal_steps > 0 ? c->num_goal_steps : 1;
  const HpScene sc = hp_scene(e, c, A.p);
  const uint32_t copies = (uint32_t)A.p.copies;
  const uint32_t gid = (uint32_t)(c->env_id_offset + m) / copies;
  const uint32_t kg = ((uint32_t)m % copies) * (uint32_t)A.S + (uint32_t)k;
  const int T = (int)(kg % (uint32_t)sc.nb);
  const float bx = sc.pos[T][0], by = sc.pos[T][1];
  const uint32_t c0 = ((uint32_t)A.p.step << 26) | (kg << 16);
  const uint32_t c3 = (RV_STREAM_PUSH_PROPOSAL << 24) | (uint32_t)A.p.plan_index;
  const int budget = A.p.max_attempts;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int found = -1;
  for (int base_att = 0; base_att < budget; base_att += 64) {
    const int att = base_att + lane;
    bool good = false;
    if (att < budget) {
      Rng g = rng_init(c->seed_lo, c->seed_hi, gid, c3, A.p.seed);
      g.c0 = c0 | ((uint32_t)att * 2u);
      good = hp_attempt(g, sc, true, 0.0f, bx, by, a);
    }
    const unsigned long long ballot = __ballot(good);
    if (ballot) { found = base_att + (int)__ffsll((long long)ballot) - 1; break; }
  }
  // the winner, or the last attempt of the budget as drawn (its lane took part in the last round)
  const int writer = found >= 0 ? (found & 63) : ((budget - 1) & 63);
  if (lane == writer) hp_write(A, G, ((size_t)m * A.S + k) * A.h + A.t, a, found >= 0 ? RV_HP_FOUND : RV_HP_EXHAUSTED);
}
#endif  // RV_ON_DEVICE

}  // namespace rv
