// Host (g++) instantiation of the view code of gym_xarm_amd/csrc/xarm_render_core.h for the CPU-side tests ONLY
// (tests/test_render_views_host.py, tests/test_render_views_gpu.py).  Never loaded by the product package: gym_xarm_amd renders
// through libxarm_hip.so (k_render_views).  Like tests/hostbuild_render it runs the kernel's scene building and per-pixel code
// without the tile culling, so an image of this build against the kernel's also checks that the culling drops nothing visible.
#define XARM_HOST_BUILD 1
#include "../../gym_xarm_amd/csrc/xarm_render_core.h"

using namespace xrc_render;

extern "C" {

int rvh_view_from_camera(const xarm_camera *cam, float *view16) {
    float v[XARM_VIEW_FLOATS];
    if (rc_view_from_camera(*cam, v)) return -1;
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) view16[k] = v[k];
    return 0;
}

int rvh_default_view(int kind, int which, float *view16) {
    float v[XARM_VIEW_FLOATS];
    if (rc_default_view(kind, which, v)) return -1;
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) view16[k] = v[k];
    return 0;
}

// rc_make_view of one record for env e of a state SoA [state_dim][stride]: returns 1 and eye, fwd, right, up (12 floats) for
// a valid view, 0 for an invalid one, -1 for an unknown kind
int rvh_make_view(int kind, int num_obj, int use_stand, const float *state, int64_t stride, int64_t e, const float *view16, int W, int H,
                  float *out12) {
    RScene sc;
    if (rc_scene_of(kind, num_obj, use_stand, sc)) return -1;
    RPrim P[MAX_PRIMS];
    RBound B[MAX_PRIMS];
    Frame<float> hands[2];
    rc_build_scene_hands(sc, state + e, stride, P, B, hands);
    RCam rc;
    if (!rc_make_view(view16, hands, sc.narms, W, H, 0, rc)) return 0;
    for (int k = 0; k < 3; k++) { out12[k] = rc.eye[k]; out12[3 + k] = rc.fwd[k]; out12[6 + k] = rc.right[k]; out12[9 + k] = rc.up[k]; }
    return 1;
}

// xarm_render_views on the host: outputs [n][V][H][W]
int rvh_render_views(int kind, int num_obj, int use_stand, const float *state, int64_t stride, int64_t num_envs, const float *views,
                     int32_t V, int32_t per_env, int32_t W, int32_t H, int32_t flags, const int32_t *ids, int32_t n, uint32_t *rgba,
                     float *depth, uint8_t *seg) {
    RScene sc;
    if (rc_scene_of(kind, num_obj, use_stand, sc)) return -1;
    const uint64_t all = sc.nprim >= 64 ? ~0ull : ((1ull << sc.nprim) - 1);
    for (int k = 0; k < n; k++) {
        const int64_t e = ids ? ids[k] : k;
        const bool env_ok = e >= 0 && e < num_envs;
        RPrim P[MAX_PRIMS];
        RBound B[MAX_PRIMS];
        Frame<float> hands[2];
        if (env_ok) rc_build_scene_hands(sc, state + e, stride, P, B, hands);
        for (int v = 0; v < V; v++) {
            const int64_t o = ((int64_t)k * V + v) * H * W;
            RCam rc;
            const bool ok = env_ok && rc_make_view(views + ((int64_t)(per_env ? k : 0) * V + v) * XARM_VIEW_FLOATS, hands, sc.narms, W, H, flags, rc);
            for (int i = 0; i < H; i++)
                for (int j = 0; j < W; j++) {
                    uint32_t c = 0u;
                    float d = 0.0f;
                    uint8_t s = SEG_INVALID;
                    if (ok) rc_pixel(P, sc.nprim, all, rc, i, j, c, d, s);
                    rgba[o + (int64_t)i * W + j] = c;
                    if (depth) depth[o + (int64_t)i * W + j] = d;
                    if (seg) seg[o + (int64_t)i * W + j] = s;
                }
        }
    }
    return 0;
}

}  // extern "C"
