// xarm_k_render.hip - k_render, the batched renderer, k_render_views, the same through device-resident view
// records (at the end of the file), and their launches.  Core: xarm_render_core.h.
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

// ---------------------------------------------------------------------------------------------------- k_render_views
// The same renderer through device-resident view records (xarm_render_core.h "views"): grid = (n * V, tiles), block x =
// k * V + v.  The first wavefront builds the primitives as k_render does and leaves each arm's hand frame in LDS; after the
// barrier thread 0 builds the RCam of (k, v) from the record and the mount's frame into LDS (rc_make_view, which also decides
// validity); after a second barrier every wavefront reads it through readfirstlane, so it sits in SGPRs and is wave-uniform
// for the culling ballot, as k_render's kernel-argument camera is.  From there on it is k_render's strip / ballot / rc_pixel
// path.  An env id out of range or an invalid view writes the invalid image (workgroup-uniform exit).  No workspace.
struct RenderViewsArgs {
    const float *state;     // [state_dim][stride]
    int64_t stride, num_envs;
    const int32_t *ids;     // [n] or null
    const float *views;     // [V][16], or [n][V][16] when per_env
    int32_t n, num_views, per_env, tiles_x, width, height, flags;
    uint32_t *rgba;         // [n][V][height][width], as depth and seg
    float *depth;
    uint8_t *seg;
    RScene sc;
};

__device__ __forceinline__ float rc_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ __launch_bounds__(256) void k_render_views(RenderViewsArgs a) {
    __shared__ RPrim prim[MAX_PRIMS];
    __shared__ RBound bound[MAX_PRIMS];
    __shared__ Frame<float> hand[2];
    __shared__ RCam scam;
    __shared__ int svalid;
    const int kv = blockIdx.x;                       // image index: k * V + v, k the position in the id list
    const int k = kv / a.num_views, v = kv - k * a.num_views;
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = (tile / a.tiles_x) * TILE + wave * 4, j0 = (tile % a.tiles_x) * TILE;
    const int i = i0 + (lane >> 4), j = j0 + (lane & 15);
    const int W = a.width, H = a.height;
    const bool inside = i < H && j < W;
    const int64_t px = ((int64_t)kv * H + i) * W + j;
    const int64_t e = a.ids ? (int64_t)a.ids[k] : (int64_t)k;
    const RScene &sc = a.sc;
    bool valid = e >= 0 && e < a.num_envs;           // workgroup-uniform: a bad env id reads no state
    if (valid) {
        if (wave == 0) {
            const float *S = a.state + e;
            if (lane < sc.narms) { rc_arm(sc, S, a.stride, lane, prim, bound); hand[lane] = rc_hand_frame(sc, S, a.stride, lane); }
            if (lane < sc.nobj) rc_object(sc, S, a.stride, lane, prim, bound);
            if (lane < sc.ngoal) rc_goal(sc, S, a.stride, lane, prim, bound);
            if (lane == 0) rc_static(sc, S, a.stride, prim, bound);
        }
        __syncthreads();
        if (tid == 0) {
            const float *view = a.views + ((int64_t)(a.per_env ? k : 0) * a.num_views + v) * XARM_VIEW_FLOATS;
            svalid = rc_make_view(view, hand, sc.narms, W, H, a.flags, scam) ? 1 : 0;
        }
        __syncthreads();
        valid = svalid != 0;
    }
    if (!valid) {
        if (inside) {
            a.rgba[px] = 0u;
            if (a.depth) a.depth[px] = 0.0f;
            if (a.seg) a.seg[px] = (uint8_t)SEG_INVALID;
        }
        return;
    }
    RCam cam;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        cam.eye[c] = rc_uniform(scam.eye[c]); cam.fwd[c] = rc_uniform(scam.fwd[c]);
        cam.right[c] = rc_uniform(scam.right[c]); cam.up[c] = rc_uniform(scam.up[c]);
    }
    cam.near_z = rc_uniform(scam.near_z); cam.far_z = rc_uniform(scam.far_z);
    cam.width = W; cam.height = H; cam.flags = a.flags;
    const bool vis = lane < sc.nprim && rc_bound_visible(bound[lane < sc.nprim ? lane : 0], cam, i0, i0 + 4, j0, j0 + TILE);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(vis);
    if (!inside) return;
    uint32_t rgba;
    float depth;
    uint8_t seg;
    rc_pixel(prim, sc.nprim, mask, cam, i, j, rgba, depth, seg);
    a.rgba[px] = rgba;
    if (a.depth) a.depth[px] = depth;
    if (a.seg) a.seg[px] = seg;
}

int launch_render_views(const float *state, int64_t stride, int64_t num_envs, const RScene &sc, const float *views, int32_t num_views,
                        int32_t per_env, int32_t width, int32_t height, int32_t flags, const int32_t *ids, int32_t n, uint32_t *rgba,
                        float *depth, uint8_t *seg, void *stream) {
    RenderViewsArgs a;
    a.state = state; a.stride = stride; a.num_envs = num_envs; a.ids = ids; a.views = views;
    a.n = n; a.num_views = num_views; a.per_env = per_env; a.width = width; a.height = height; a.flags = flags;
    a.tiles_x = (width + TILE - 1) / TILE;
    a.rgba = rgba; a.depth = depth; a.seg = seg; a.sc = sc;
    const int tiles_y = (height + TILE - 1) / TILE;
    k_render_views<<<dim3((unsigned)n * (unsigned)num_views, (unsigned)(a.tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace xrc_render
