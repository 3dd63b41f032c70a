// rv_dev_contacts.h — PyBullet contact records of every env on the device (rv_get_contact_points).
//
// Reference: BulletPhysics.get_contact_points (robovat/simulation/physics/bullet_physics.py:1262-1304), i.e.
// pybullet.getContactPoints, which Simulator.check_contact (robovat/simulation/simulator.py:246-287) and Body.contacts
// read.  One record per point of a persistent manifold, in PyBullet's field order:
//   ids  int32[4]         bodyA, bodyB, linkA, linkB
//   data float[RV_CP_NF]  positionOnA[3], positionOnB[3], contactNormalOnB[3], contactDistance, normalForce,
//                         lateralFriction1, lateralFrictionDir1[3], lateralFriction2, lateralFrictionDir2[3]
//
// Body codes: a body slot 0..RV_MAXB-1 (movable or static), RV_CP_TABLE = RV_MAXB, RV_CP_ARM = RV_MAXB + 1 (the
// segmask convention of rv_render).  Links: -1 for a body or the table, arm->col_frame[col] (a scenes.LINK_NAMES
// index) for an arm point.
//
// Launch: one wave64 per env, lane l = 4 mi + i is point i of manifold slot mi, read straight from the DevEnv in
// global memory (nothing is staged in LDS); lane RV_NMAN * 4 is the arm-table record.  Which points are records is
// gated on the words the hit test of rv_query_contacts / rv_get_manifold_counts reads, so for every pair of
// entities "the list is non-empty" is the old answer of HipPhysics.get_contact_points:
//   body-table RV_TIDX(b), body-body RV_BBIDX(k): every point i < n (the manifold is non-empty).  A body entirely
//     below the table keeps its contacts with the ground in its table slot: they are reported with the table as
//     body B, as the hit test reports them.
//   arm-body RV_AIDX(b): only while e.active[b] && e.flag_arm_body[b], and then only the points with
//     dist < contact_query_dist -- the rule that forms the flag (rv_dev_env.h, the flag update after the narrow
//     phase).  Coasting substeps clear the flag, so arm records vanish exactly when check_contact says no.
//   arm-table: a collider flag, not a manifold.  While e.flag_arm_table is set one record follows all manifold
//     records: bodyA = arm, bodyB = table, both links -1, NaN positions and distance, normal +z, zero forces.  A
//     link filter on the arm matches it (the flag does not say which link touched).
//
// Quantities: positionOnA = A's pose applied to la; positionOnB = B's frame applied to lb (the table: world
// coordinates; another body: its pose; the arm: the link frame of the collider).  The normal points from B to A,
// and the solver pushes A with +ln along it and +lt1, +lt2 along plane_space(normal) (row_setup: the body velocity
// grows by ima * lambda * dir), so the net contact force on A is fn n + f1 d1 + f2 d2, with f = impulse / dt.  The
// impulses are the ones the last solve of the pair left: a sleeping body reports those of its last solve, as a
// sleeping Bullet manifold keeps its applied impulses.
//
// Query (rv_contact_query, -1 = any): a record matches when its two sides match the two sides of the query, in
// either order.  A record is oriented so that the query's body_a is its A (else, if the query names only body_b,
// so that body_b is its B): a swap exchanges the positions and the links and negates n, d1 and d2; the magnitudes
// stay.  Records are compacted in a stable order (manifold slot, point, then the arm-table record) with a ballot;
// count[env] is the number of matches, of which the first `capacity` are written.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"
#include "rv_dev_env.h"

#define RV_CP_WAVES 4   // envs (waves) per workgroup

namespace rv {

static_assert(RV_NMAN * 4 <= 64, "one lane per manifold point");
static_assert(RV_NMAN * 4 + 1 <= 64, "the arm-table record needs a lane of its own");
static_assert(RV_CP_MAX == RV_NMAN * 4 + 1, "rovat.h: RV_CP_MAX");

struct CpArgs {
  rv_contact_query q;
  int capacity;
  int32_t* ids;     // [N][capacity][4]
  float* data;      // [N][capacity][RV_CP_NF]
  int32_t* count;   // [N]
};

// does (body, link) of one side of a record pass (qb, ql) of the query?  (ql >= 0 only with qb == the arm; the
// arm-table record has link -1 and passes every link of the arm)
RV_DEV bool cp_side_match(int qb, int ql, int body, int link) {
  return (qb < 0 || qb == body) && (ql < 0 || link < 0 || link == ql);
}

__global__ __launch_bounds__(64 * RV_CP_WAVES) void k_contact_points(const DevEnv* envs, int n, const rv_config* c, const rv_scene* scene, CpArgs A) {
  const int env = (int)blockIdx.x * RV_CP_WAVES + (int)threadIdx.x / 64;
  if (env >= n) return;      // (wave-uniform)
  const int lane = (int)threadIdx.x & 63;
  const DevEnv& e = envs[env];
  const rv_arm* arm = &scene->arm;

  int ba = -1, bb = -1, lka = -1, lkb = -1;
  v3 pa = mk(0.0f, 0.0f, 0.0f), pb = pa, nrm = mk(0.0f, 0.0f, 1.0f);
  float dist = 0.0f, fn = 0.0f, f1 = 0.0f, f2 = 0.0f;
  bool rec = false;
  if (lane < RV_NMAN * 4) {
    const int mi = lane >> 2, i = lane & 3;
    const DevMan& m = e.man[mi];
    int kind, a, b;
    man_owner(mi, &kind, &a, &b);
    rec = i < m.n;
    if (kind == 2) rec = rec && e.active[a] && e.flag_arm_body[a] && m.dist[i] < c->contact_query_dist;
    if (rec) {
      ba = a;
      pa = add(ld3(e.body[a]), mulv(qmat(ldq(e.body[a] + 3)), ld3(m.la[i])));
      const v3 lb = ld3(m.lb[i]);
      if (kind == 0) { bb = RV_CP_TABLE; pb = lb; }
      else if (kind == 1) { bb = b; pb = add(ld3(e.body[b]), mulv(qmat(ldq(e.body[b] + 3)), lb)); }
      else {
        const int f = arm->col_frame[m.col[i]];
        bb = RV_CP_ARM; lkb = f;
        pb = add(ld3(e.fpos[f]), mulv(qmat(ldq(e.fquat[f])), lb));
      }
      nrm = ld3(m.nrm[i]);
      dist = m.dist[i];
      const float inv_dt = 1.0f / c->dt;
      fn = m.ln[i] * inv_dt; f1 = m.lt1[i] * inv_dt; f2 = m.lt2[i] * inv_dt;
    }
  } else if (lane == RV_NMAN * 4 && e.flag_arm_table) {
    rec = true;
    ba = RV_CP_ARM; bb = RV_CP_TABLE;
    const float qnan = __builtin_nanf("");
    pa = mk(qnan, qnan, qnan); pb = pa; dist = qnan;
  }
  v3 d1, d2;
  plane_space(nrm, &d1, &d2);

  // the query: orientation first, then both sides
  const rv_contact_query& q = A.q;
  const bool swap = q.body_a >= 0 ? (bb == q.body_a && ba != q.body_a) : (q.body_b >= 0 && ba == q.body_b && bb != q.body_b);
  if (swap) {
    int t = ba; ba = bb; bb = t;
    t = lka; lka = lkb; lkb = t;
    v3 p = pa; pa = pb; pb = p;
    nrm = scale(nrm, -1.0f); d1 = scale(d1, -1.0f); d2 = scale(d2, -1.0f);
  }
  const bool match = rec && cp_side_match(q.body_a, q.link_a, ba, lka) && cp_side_match(q.body_b, q.link_b, bb, lkb);

  // stable compaction: slot = number of matching lanes below this one
  const unsigned long long mask = __ballot(match);
  const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  if (lane == 0) A.count[env] = __popcll(mask);
  if (match && slot < A.capacity) {
    const size_t r = (size_t)env * (size_t)A.capacity + (size_t)slot;
    int32_t* id = A.ids + r * 4;
    id[0] = ba; id[1] = bb; id[2] = lka; id[3] = lkb;
    float* o = A.data + r * RV_CP_NF;
    st3(o + 0, pa); st3(o + 3, pb); st3(o + 6, nrm);
    o[9] = dist; o[10] = fn;
    o[11] = f1; st3(o + 12, d1);
    o[15] = f2; st3(o + 16, d2);
  }
}

}  // namespace rv
