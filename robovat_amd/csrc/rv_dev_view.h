// rv_dev_view.h -- free camera views of chosen envs, the kernel of rv_render_view (include/rovat.h).
// A stand-alone kernel beside the env program; it includes rv_dev_env.h for ObsSnap and the ray caster of rv_dev_obs.h
// (render_pixel, shade_rgb), which it calls and does not restate.
//
// One pixel.  View k looks at env env_index[k] through camera row k (fx, fy, cx, cy, skew, rotation[9], translation[3]).
// Its pixel (u, v) is what k_render / k_render_rgb (rv_kernels.hip) compute for that env with the camera fields of the
// env's ObsSnap replaced by the row: pixel_dir_cam at ((float)u, (float)v), cam_to_world_dir, cam_position, render_pixel,
// the cam_near cut, shade_rgb -- the same functions on the same values in the same order, so the same bits (the library
// is compiled with -ffp-contract=off: an expression rounds the same wherever it is inlined).  With supersample = s > 1
// the row arrives scaled to the s-times larger image (rv_render_view does that on the host) and output pixel (u, v) is
// (sum + s s / 2) / (s s), per channel and in integers, over the s x s pixels (s u + i, s v + j) of that image.
//
// Shape.  256 threads per workgroup; a workgroup belongs to ONE view (blockIdx.y) and draws 1024 consecutive pixels of it,
// four per thread, 256 apart (consecutive lanes, consecutive pixels).  What k_render computes once per thread -- the four
// body rotation matrices and the camera origin -- is computed once per workgroup into LDS, next to the view's copy of the
// snapshot with the row in place (676 bytes in all), and every thread reads it from there.  (With ONE pixel per thread the
// three barriers of that prologue cost more than they saved: 13 % slower than k_render_rgb at 64 x 424 x 512, DESIGN.md
// §23.)  The ten arm box rotations stay inside render_pixel: calling it is the contract, and it computes them after its
// bounding-sphere test, only for the boxes a ray comes near.  No atomics; the outputs leave by ordinary vector stores;
// every global index is a size_t.
#ifndef RV_DEV_VIEW_H_
#define RV_DEV_VIEW_H_
#include "rv_dev_env.h"

#define RV_VIEW_TPB 256
#define RV_VIEW_PPT 4      // pixels per thread: a workgroup draws RV_VIEW_TPB * RV_VIEW_PPT consecutive pixels of its view

namespace rv {
struct ViewArgs {
  const ObsSnap* snaps;        // [N]: k_obs_snap of the envs as they are now
  const int32_t* env_index;    // [V]
  const float* cameras;        // [V][17], scaled by `ss` already
  int height, width, ss;
  uint8_t* rgb;                // [V][height][width][3] or nullptr
  float* depth;                // [V][height][width] or nullptr (ss == 1)
  uint8_t* seg;                // [V][height][width] or nullptr (ss == 1)
};

static_assert(sizeof(ObsSnap) % sizeof(uint32_t) == 0, "ObsSnap is copied word by word");

#if RV_ON_DEVICE
__global__ __launch_bounds__(RV_VIEW_TPB) void k_render_view(ViewArgs a, const rv_config* c, const rv_scene* scene) {
  __shared__ ObsSnap s_snap;
  __shared__ float s_rot[RV_MAXB][9];
  __shared__ float s_cam_o[3];
  const int tid = (int)threadIdx.x;
  const size_t view = (size_t)blockIdx.y;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.snaps + a.env_index[view]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s_snap);
    for (int i = tid; i < (int)(sizeof(ObsSnap) / sizeof(uint32_t)); i += RV_VIEW_TPB) dst[i] = src[i];
  }
  __syncthreads();
  {
    const float* row = a.cameras + view * 17;
    if (tid < 5) s_snap.cam_intrinsics[tid] = row[tid];
    else if (tid < 14) s_snap.cam_rotation[tid - 5] = row[tid];
    else if (tid < 17) s_snap.cam_translation[tid - 14] = row[tid];
  }
  __syncthreads();
  if (tid < RV_MAXB) { m3 m = qmat(ldq(s_snap.pose[tid] + 3)); stm(s_rot[tid], m); }
  if (tid == 64) { const v3 o = cam_position(&s_snap); s_cam_o[0] = o.x; s_cam_o[1] = o.y; s_cam_o[2] = o.z; }
  __syncthreads();
  const int H = a.height, W = a.width, ss = a.ss;
  const v3 cam_o = mk(s_cam_o[0], s_cam_o[1], s_cam_o[2]);
  for (int k = 0; k < RV_VIEW_PPT; ++k) {
    const int px = ((int)blockIdx.x * RV_VIEW_PPT + k) * RV_VIEW_TPB + tid;      // (H W <= 2^24)
    if (px >= H * W) break;
    const int v = px / W, u = px - v * W;
    int sum[3] = {0, 0, 0};
    float d = 0.0f; int who = -1;
    for (int j = 0; j < ss; ++j) {
      for (int i = 0; i < ss; ++i) {
        v3 nrm;
        who = render_pixel(c, scene, s_snap, s_rot, cam_o,
                           cam_to_world_dir(&s_snap, pixel_dir_cam(&s_snap, (float)(ss * u + i), (float)(ss * v + j))), &d, &nrm);
        if (who >= 0 && !(d > c->cam_near)) who = -1;
        uint8_t col[3];
        shade_rgb(who, nrm, col);
        sum[0] += col[0]; sum[1] += col[1]; sum[2] += col[2];
      }
    }
    const size_t t = view * (size_t)H * (size_t)W + (size_t)px;
    if (a.rgb) {
      const int n = ss * ss, half = n / 2;
      uint8_t* o = a.rgb + t * 3;
      o[0] = (uint8_t)((sum[0] + half) / n); o[1] = (uint8_t)((sum[1] + half) / n); o[2] = (uint8_t)((sum[2] + half) / n);
    }
    // (ss == 1 when either is given: `who` and `d` are the one pixel's)
    if (a.depth) a.depth[t] = who >= 0 ? d : 0.0f;
    if (a.seg) a.seg[t] = who >= 0 ? (uint8_t)who : (uint8_t)255;
  }
}
#endif

}  // namespace rv
#endif
