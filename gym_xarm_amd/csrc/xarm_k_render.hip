// xarm_k_render.hip - k_render, the batched renderer, and its launch.  Core: xarm_render_core.h.
//
// One workgroup of 256 threads per (env, 16 x 16 tile): grid = (n, tiles).  The first wavefront rebuilds the env's primitives
// into LDS from the state (arm FK in one lane per arm, one lane per object / goal, the static scene in lane 0) - ~1 kFLOP
// against ~200 kFLOP of pixel work per tile, so it is recomputed per tile rather than shared.  After the barrier each wavefront
// owns a 16 x 4 pixel strip: lane p tests primitive p's bounding sphere against the strip's frustum and the 64-bit ballot of
// the survivors is the (wave-uniform, SGPR) list the per-pixel loop walks (s_ff1).  Every lane stores one uint32 of RGBA and,
// when asked, one float of depth and one byte of segmentation.  Nothing is allocated per call; the state is only read.
#include <hip/hip_runtime.h>
#include "xarm_render_core.h"

namespace xrc_render {

struct RenderArgs {
    const float *state;     // [state_dim][stride]
    int64_t stride, num_envs;
    const int32_t *ids;     // [n] or null
    int32_t n, tiles_x;
    uint32_t *rgba;
    float *depth;
    uint8_t *seg;
    RScene sc;
    RCam cam;
};

__global__ __launch_bounds__(256) void k_render(RenderArgs a) {
    __shared__ RPrim prim[MAX_PRIMS];
    __shared__ RBound bound[MAX_PRIMS];
    const int k = blockIdx.x;                        // position in the id list
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = (tile / a.tiles_x) * TILE + wave * 4, j0 = (tile % a.tiles_x) * TILE;
    const int i = i0 + (lane >> 4), j = j0 + (lane & 15);
    const int W = a.cam.width, H = a.cam.height;
    const bool inside = i < H && j < W;
    const int64_t px = ((int64_t)k * H + i) * W + j;
    const int64_t e = a.ids ? (int64_t)a.ids[k] : (int64_t)k;
    if (e < 0 || e >= a.num_envs) {                  // workgroup-uniform: no primitive is read
        if (inside) {
            a.rgba[px] = 0u;
            if (a.depth) a.depth[px] = 0.0f;
            if (a.seg) a.seg[px] = (uint8_t)SEG_INVALID;
        }
        return;
    }
    const RScene &sc = a.sc;
    if (wave == 0) {
        const float *S = a.state + e;
        if (lane < sc.narms) rc_arm(sc, S, a.stride, lane, prim, bound);
        if (lane < sc.nobj) rc_object(sc, S, a.stride, lane, prim, bound);
        if (lane < sc.ngoal) rc_goal(sc, S, a.stride, lane, prim, bound);
        if (lane == 0) rc_static(sc, S, a.stride, prim, bound);
    }
    __syncthreads();
    const bool vis = lane < sc.nprim && rc_bound_visible(bound[lane < sc.nprim ? lane : 0], a.cam, i0, i0 + 4, j0, j0 + TILE);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(vis);
    if (!inside) return;
    uint32_t rgba;
    float depth;
    uint8_t seg;
    rc_pixel(prim, sc.nprim, mask, a.cam, i, j, rgba, depth, seg);
    a.rgba[px] = rgba;
    if (a.depth) a.depth[px] = depth;
    if (a.seg) a.seg[px] = seg;
}

int launch_render(const float *state, int64_t stride, int64_t num_envs, const RScene &sc, const RCam &cam, const int32_t *ids, int32_t n,
                  uint32_t *rgba, float *depth, uint8_t *seg, void *stream) {
    RenderArgs a;
    a.state = state; a.stride = stride; a.num_envs = num_envs; a.ids = ids; a.n = n;
    a.tiles_x = (cam.width + TILE - 1) / TILE;
    a.rgba = rgba; a.depth = depth; a.seg = seg; a.sc = sc; a.cam = cam;
    const int tiles_y = (cam.height + TILE - 1) / TILE;
    k_render<<<dim3((unsigned)n, (unsigned)(a.tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace xrc_render
