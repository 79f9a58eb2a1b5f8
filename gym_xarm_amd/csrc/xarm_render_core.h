// xarm_render_core.h - per-environment render core: the scene of one env as <= 64 primitives, and one camera ray per pixel
// cast against them.  Read-only on the simulator state: nothing here writes it.
//
// Like the physics cores this compiles for gfx950 (hipcc; the kernel is xarm_k_render.hip) and, for the CPU tests only, for
// the host (g++ -DXARM_HOST_BUILD, tests/hostbuild_render/).  The arm frames come from the physics cores' own FK
// (xk::fk_advance and the per-arm base frames of the Handover / StackTower scenes), in float32.
//
//   scene     per arm: 7 link capsules (the segments between consecutive joint origins; the two zero-length ones are
//             spheres) + the hand box and the two finger boxes (Panda gripper) or one gripper box (Reach's xArm gripper);
//             then one box per object, one sphere per goal marker, the ground plane, the table top(s) and the Handover stand.
//   ray       box by slabs in its local frame, capsule / sphere by their quadratics, the ground by its plane; the nearest
//             hit in [near, far] wins, ties to the lower primitive index.  One ray per pixel centre, no anti-aliasing.
//   shading   Lambert from one directional light + ambient, optionally a shadow ray against every primitive
//             (XARM_RENDER_SHADOWS).  Outputs: RGBA8 in one uint32 (alpha 255), the view-axis depth in metres (far for the
//             background), the segmentation class (table 1, arm a links 2 + 2a / gripper 3 + 2a, object k 8 + k, goal k 16 + k;
//             k < 4).
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/xarm_hip.h"
#include "xarm_core.h"
#include "xarm_reach_core.h"
#include "xarm_handover_core.h"
#include "xarm_handover2_core.h"
#include "xarm_stack_core.h"
#include "xarm_rearrange_core.h"
#include "xarm_render_model.h"

namespace xrc_render {

using xk::V3;
using xk::mk;
using xk::Frame;

constexpr int MAX_PRIMS = 64;
constexpr int TILE = 16;                         // a workgroup renders a 16 x 16 tile, each of its 4 wavefronts 16 x 4 pixels
enum { P_BOX = 0, P_CAPSULE = 1, P_SPHERE = 2, P_PLANE = 3 };
// palette indices (xarm_render_model.h PALETTE, tools/gen_render_header.py)
enum { C_BACKGROUND = 0, C_TABLE = 1, C_GROUND = 2, C_STAND = 3, C_ARM = 4, C_GRIPPER = 5, C_ARM1 = 6, C_GRIPPER1 = 7, C_OBJ = 8, C_GOAL = 11,
       C_OBJ3 = 14, C_GOAL3 = 15 };   // object / goal 3: Rearrange's fourth cube
enum { SEG_BACKGROUND = 0, SEG_TABLE = 1, SEG_ARM = 2, SEG_OBJ = 8, SEG_GOAL = 16, SEG_INVALID = 255 };
constexpr float RC_INF = 3.0e38f;

// 64 B: box c[0..2] R columns [3..11] half [12..14]; capsule a[0..2] b[3..5] r[6]; sphere c[0..2] r[6]; plane z[2];
// v[15] = type + 4 * palette + 64 * seg (small integers, exact in float32)
struct RPrim { float v[16]; };
// bounding sphere for the tile culling: centre, radius (< 0: unbounded - the plane)
struct RBound { float c[4]; };

// camera in closed form (rc_make_camera): ray through pixel (i, j) = fwd + right * x + up * y, x, y the pixel centre in NDC;
// right / up carry tan(fov / 2) (x aspect), so the ray parameter t IS the view-axis depth (dot(ray, fwd) = 1)
struct RCam {
    float eye[3], fwd[3], right[3], up[3];
    float near_z, far_z;
    int width, height, flags;
};

// where a scene's fields live in the state (SoA [field][stride]) and how many primitives of each kind it has
struct RScene {
    int kind, narms, arm_prims, nobj, ngoal, nstatic, nprim, use_stand;
    int q_off, bp_off, bq_off, goal_off;
    float obj_half[3], goal_radius;
};

XARM_HD float rc_meta(int type, int pal, int seg) { return (float)(type + 4 * pal + 64 * seg); }
XARM_HD int rc_type(float m) { return (int)m & 3; }
XARM_HD int rc_pal(float m) { return ((int)m >> 2) & 15; }
XARM_HD int rc_seg(float m) { return (int)m >> 6; }

XARM_HD void rc_box(RPrim &p, RBound &b, V3<float> c, V3<float> c0, V3<float> c1, V3<float> c2, const float (&h)[3], int pal, int seg) {
    p.v[0] = c.x; p.v[1] = c.y; p.v[2] = c.z;
    p.v[3] = c0.x; p.v[4] = c0.y; p.v[5] = c0.z; p.v[6] = c1.x; p.v[7] = c1.y; p.v[8] = c1.z; p.v[9] = c2.x; p.v[10] = c2.y; p.v[11] = c2.z;
    p.v[12] = h[0]; p.v[13] = h[1]; p.v[14] = h[2]; p.v[15] = rc_meta(P_BOX, pal, seg);
    b.c[0] = c.x; b.c[1] = c.y; b.c[2] = c.z; b.c[3] = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
}
// box given by its local corners lo / hi in the frame f
XARM_HD void rc_box_local(RPrim &p, RBound &b, const Frame<float> &f, const float (&lo)[3], const float (&hi)[3], int pal, int seg) {
    const float h[3] = {0.5f * (hi[0] - lo[0]), 0.5f * (hi[1] - lo[1]), 0.5f * (hi[2] - lo[2])};
    const V3<float> c = f.o + f.c0 * (0.5f * (hi[0] + lo[0])) + f.c1 * (0.5f * (hi[1] + lo[1])) + f.c2 * (0.5f * (hi[2] + lo[2]));
    rc_box(p, b, c, f.c0, f.c1, f.c2, h, pal, seg);
}
XARM_HD void rc_sphere(RPrim &p, RBound &b, V3<float> c, float r, int pal, int seg) {
#pragma unroll
    for (int k = 0; k < 16; k++) p.v[k] = 0.0f;
    p.v[0] = c.x; p.v[1] = c.y; p.v[2] = c.z; p.v[6] = r; p.v[15] = rc_meta(P_SPHERE, pal, seg);
    b.c[0] = c.x; b.c[1] = c.y; b.c[2] = c.z; b.c[3] = r;
}
XARM_HD void rc_capsule(RPrim &p, RBound &b, V3<float> a, V3<float> e, float r, int pal, int seg) {
    const V3<float> d = e - a;
    const float l2 = xk::dot(d, d);
    if (l2 < 1e-12f) { rc_sphere(p, b, a, r, pal, seg); return; }   // link2 / link6: the joint origins coincide
#pragma unroll
    for (int k = 0; k < 16; k++) p.v[k] = 0.0f;
    p.v[0] = a.x; p.v[1] = a.y; p.v[2] = a.z; p.v[3] = e.x; p.v[4] = e.y; p.v[5] = e.z; p.v[6] = r;
    p.v[15] = rc_meta(P_CAPSULE, pal, seg);
    b.c[0] = 0.5f * (a.x + e.x); b.c[1] = 0.5f * (a.y + e.y); b.c[2] = 0.5f * (a.z + e.z); b.c[3] = 0.5f * sqrtf(l2) + r;
}

// ---------------------------------------------------------------------------------------------------- scene building
XARM_HD Frame<float> rc_base_frame(int kind, int arm) {
    if (kind == XARM_ENV_HANDOVER) return xh::HandoverScene::base_frame<float>(arm);
    if (kind == XARM_ENV_STACK_TOWER || kind == XARM_ENV_REARRANGE) return xs::StackScene::base_frame<float>(arm);
    return xk::frame_identity<float>();
}

// primitives [arm * arm_prims, (arm + 1) * arm_prims) of the env whose state column starts at S
XARM_HD void rc_arm(const RScene &sc, const float *S, int64_t n, int arm, RPrim *P, RBound *B) {
    const int base = arm * sc.arm_prims;
    const int seg_l = SEG_ARM + 2 * arm, seg_g = seg_l + 1;
    const int pal_l = arm == 0 ? C_ARM : C_ARM1, pal_g = arm == 0 ? C_GRIPPER : C_GRIPPER1;
    Frame<float> f = rc_base_frame(sc.kind, arm);
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const V3<float> o = f.o;
        xk::fk_advance(f, i, S[(sc.q_off + 9 * arm + i) * n]);
        rc_capsule(P[base + i], B[base + i], o, f.o, xrm::LINK_RADIUS[i], pal_l, seg_l);
    }
    // hand frame = link7 frame (link_eef and the hand / gripper base are fixed, zero offset)
    if (sc.kind == XARM_ENV_REACH) {
        rc_box_local(P[base + 7], B[base + 7], f, xrm::REACH_GRIPPER_LO, xrm::REACH_GRIPPER_HI, pal_g, seg_g);
        return;
    }
    rc_box_local(P[base + 7], B[base + 7], f, xrm::HAND_LO, xrm::HAND_HI, pal_g, seg_g);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float sg = k == 0 ? 1.0f : -1.0f;
        Frame<float> ff = f;
        ff.o = f.o + f.c2 * xrm::FINGER_Z + f.c1 * (sg * S[(sc.q_off + 9 * arm + 7 + k) * n]);
        // right finger: y sign flipped (collision mesh yaw pi)
        const float lo[3] = {xrm::FINGER_LO[0], k == 0 ? xrm::FINGER_LO[1] : -xrm::FINGER_HI[1], xrm::FINGER_LO[2]};
        const float hi[3] = {xrm::FINGER_HI[0], k == 0 ? xrm::FINGER_HI[1] : -xrm::FINGER_LO[1], xrm::FINGER_HI[2]};
        rc_box_local(P[base + 8 + k], B[base + 8 + k], ff, lo, hi, pal_g, seg_g);
    }
}
// the hand frame of an arm: the link-7 frame rc_arm ends its FK with (+z to the fingertips, the fingers slide along y; Reach:
// the same frame under the xArm gripper box) - the mount of a wrist view.  The same calls in the same order as rc_arm's, apart
// from it so that rc_arm, and with it k_render's code, stays as it is.
XARM_HD Frame<float> rc_hand_frame(const RScene &sc, const float *S, int64_t n, int arm) {
    Frame<float> f = rc_base_frame(sc.kind, arm);
#pragma unroll
    for (int i = 0; i < 7; i++) xk::fk_advance(f, i, S[(sc.q_off + 9 * arm + i) * n]);
    return f;
}

XARM_HD void rc_object(const RScene &sc, const float *S, int64_t n, int k, RPrim *P, RBound *B) {
    const int slot = sc.narms * sc.arm_prims + k;
    const V3<float> c = mk<float>(S[(sc.bp_off + 3 * k) * n], S[(sc.bp_off + 3 * k + 1) * n], S[(sc.bp_off + 3 * k + 2) * n]);
    const float x = S[(sc.bq_off + 4 * k) * n], y = S[(sc.bq_off + 4 * k + 1) * n], z = S[(sc.bq_off + 4 * k + 2) * n],
                w = S[(sc.bq_off + 4 * k + 3) * n];
    // quaternion (x, y, z, w) -> rotation matrix columns
    const V3<float> c0 = mk<float>(1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y + w * z), 2.0f * (x * z - w * y));
    const V3<float> c1 = mk<float>(2.0f * (x * y - w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z + w * x));
    const V3<float> c2 = mk<float>(2.0f * (x * z + w * y), 2.0f * (y * z - w * x), 1.0f - 2.0f * (x * x + y * y));
    const float h[3] = {sc.obj_half[0], sc.obj_half[1], sc.obj_half[2]};
    rc_box(P[slot], B[slot], c, c0, c1, c2, h, k < 3 ? C_OBJ + k : C_OBJ3, SEG_OBJ + k);
}

XARM_HD V3<float> rc_goal_pos(const RScene &sc, const float *S, int64_t n, int k) {
    return mk<float>(S[(sc.goal_off + 3 * k) * n], S[(sc.goal_off + 3 * k + 1) * n], S[(sc.goal_off + 3 * k + 2) * n]);
}

XARM_HD void rc_goal(const RScene &sc, const float *S, int64_t n, int k, RPrim *P, RBound *B) {
    const int slot = sc.narms * sc.arm_prims + sc.nobj + k;
    rc_sphere(P[slot], B[slot], rc_goal_pos(sc, S, n, k), sc.goal_radius, k < 3 ? C_GOAL + k : C_GOAL3, SEG_GOAL + k);
}

// ground plane, table top(s), the Handover stand
XARM_HD void rc_static(const RScene &sc, const float *S, int64_t n, RPrim *P, RBound *B) {
    int s = sc.narms * sc.arm_prims + sc.nobj + sc.ngoal;
#pragma unroll
    for (int k = 0; k < 16; k++) P[s].v[k] = 0.0f;
    P[s].v[2] = xrm::GROUND_Z; P[s].v[15] = rc_meta(P_PLANE, C_GROUND, SEG_TABLE);
    B[s].c[0] = B[s].c[1] = B[s].c[2] = 0.0f; B[s].c[3] = -1.0f;
    s++;
    const V3<float> ex = mk<float>(1.0f, 0.0f, 0.0f), ey = mk<float>(0.0f, 1.0f, 0.0f), ez = mk<float>(0.0f, 0.0f, 1.0f);
    const float tz = xrm::TABLE_TOP_Z - 0.5f * xrm::TABLE_THICKNESS;
    if (sc.kind == XARM_ENV_HANDOVER) {
        const float hx = 0.5f * (xrm::HO_TABLE_X_MAX - xrm::HO_TABLE_X_MIN), cx = 0.5f * (xrm::HO_TABLE_X_MAX + xrm::HO_TABLE_X_MIN);
        const float h[3] = {hx, xrm::HO_TABLE_HALF_Y, 0.5f * xrm::TABLE_THICKNESS};
        rc_box(P[s], B[s], mk<float>(-cx, 0.0f, tz), ex, ey, ez, h, C_TABLE, SEG_TABLE);
        rc_box(P[s + 1], B[s + 1], mk<float>(cx, 0.0f, tz), ex, ey, ez, h, C_TABLE, SEG_TABLE);
        s += 2;
        if (sc.use_stand) {   // xarm_handover.py:391-392: the stand's top sits stand_below_goal - stand_half_z under goal 0
            const V3<float> g = rc_goal_pos(sc, S, n, 0);
            const float sh[3] = {xrm::HO_STAND_HALF[0], xrm::HO_STAND_HALF[1], xrm::HO_STAND_HALF[2]};
            rc_box(P[s], B[s], mk<float>(g.x, g.y, g.z - xrm::HO_STAND_BELOW_GOAL), ex, ey, ez, sh, C_STAND, SEG_TABLE);
        }
    } else {
        const float h[3] = {xrm::TABLE_HALF_X, xrm::TABLE_HALF_Y, 0.5f * xrm::TABLE_THICKNESS};
        rc_box(P[s], B[s], mk<float>(0.0f, 0.0f, tz), ex, ey, ez, h, C_TABLE, SEG_TABLE);
    }
}

// every primitive of one env (the host build; the kernel spreads the same calls over the lanes of its first wavefront)
XARM_HD void rc_build_scene(const RScene &sc, const float *S, int64_t n, RPrim *P, RBound *B) {
    for (int a = 0; a < sc.narms; a++) rc_arm(sc, S, n, a, P, B);
    for (int k = 0; k < sc.nobj; k++) rc_object(sc, S, n, k, P, B);
    for (int k = 0; k < sc.ngoal; k++) rc_goal(sc, S, n, k, P, B);
    rc_static(sc, S, n, P, B);
}
// the same, keeping the hand frame of every arm (hands[0 .. narms)) for the mounted views
XARM_HD void rc_build_scene_hands(const RScene &sc, const float *S, int64_t n, RPrim *P, RBound *B, Frame<float> *hands) {
    for (int a = 0; a < sc.narms; a++) { rc_arm(sc, S, n, a, P, B); hands[a] = rc_hand_frame(sc, S, n, a); }
    for (int k = 0; k < sc.nobj; k++) rc_object(sc, S, n, k, P, B);
    for (int k = 0; k < sc.ngoal; k++) rc_goal(sc, S, n, k, P, B);
    rc_static(sc, S, n, P, B);
}

// ---------------------------------------------------------------------------------------------------- ray casting
XARM_HD V3<float> rc_v(const float *p) { return mk<float>(p[0], p[1], p[2]); }

// nearest t >= tmin of the ray o + t d (d not normalised) with primitive p, RC_INF for none
XARM_HD float rc_intersect(const RPrim &p, V3<float> o, V3<float> d, float tmin) {
    const int type = rc_type(p.v[15]);
    const V3<float> c = rc_v(p.v);
    if (type == P_BOX) {
        const V3<float> r = o - c;
        const V3<float> ax[3] = {rc_v(p.v + 3), rc_v(p.v + 6), rc_v(p.v + 9)};
        float t0 = -RC_INF, t1 = RC_INF;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float lo = xk::dot(ax[k], r), ld = xk::dot(ax[k], d), h = p.v[12 + k];
            const float inv = 1.0f / ld;
            const float ta = (-h - lo) * inv, tb = (h - lo) * inv;
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        }
        if (t1 < t0) return RC_INF;
        return t0 >= tmin ? t0 : (t1 >= tmin ? t1 : RC_INF);
    }
    if (type == P_PLANE) {
        const float t = (p.v[2] - o.z) / d.z;
        return t >= tmin ? t : RC_INF;
    }
    const float r = p.v[6], dd = xk::dot(d, d);
    if (type == P_SPHERE) {
        const V3<float> oc = o - c;
        const float b = xk::dot(oc, d), cc = xk::dot(oc, oc) - r * r, h = b * b - dd * cc;
        if (h < 0.0f) return RC_INF;
        const float t = (-b - sqrtf(h)) / dd;
        return t >= tmin ? t : RC_INF;
    }
    // capsule a = c, b = v[3..5]
    const V3<float> e = rc_v(p.v + 3), ba = e - c, oa = o - c;
    const float baba = xk::dot(ba, ba), bard = xk::dot(ba, d), baoa = xk::dot(ba, oa), rdoa = xk::dot(d, oa), oaoa = xk::dot(oa, oa);
    const float qa = baba * dd - bard * bard, qb = baba * rdoa - baoa * bard, qc = baba * oaoa - baoa * baoa - r * r * baba;
    const float h = qb * qb - qa * qc;
    if (h < 0.0f) return RC_INF;
    float t = (-qb - sqrtf(h)) / qa;
    const float y = baoa + t * bard;
    if (y > 0.0f && y < baba) return t >= tmin ? t : RC_INF;
    // end caps
    const V3<float> oc = y <= 0.0f ? oa : o - e;
    const float b2 = xk::dot(d, oc), c2 = xk::dot(oc, oc) - r * r, h2 = b2 * b2 - dd * c2;
    if (h2 < 0.0f) return RC_INF;
    t = (-b2 - sqrtf(h2)) / dd;
    return t >= tmin ? t : RC_INF;
}

// outward normal of primitive p at the surface point x
XARM_HD V3<float> rc_normal(const RPrim &p, V3<float> x) {
    const int type = rc_type(p.v[15]);
    const V3<float> c = rc_v(p.v);
    if (type == P_PLANE) return mk<float>(0.0f, 0.0f, 1.0f);
    V3<float> n;
    if (type == P_BOX) {
        const V3<float> r = x - c;
        const V3<float> ax[3] = {rc_v(p.v + 3), rc_v(p.v + 6), rc_v(p.v + 9)};
        int best = 0;
        float bv = -1.0f, bs = 1.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float l = xk::dot(ax[k], r), q = fabsf(l) / p.v[12 + k];
            if (q > bv) { bv = q; best = k; bs = l < 0.0f ? -1.0f : 1.0f; }
        }
        return ax[best] * bs;
    }
    if (type == P_SPHERE) n = x - c;
    else {
        const V3<float> ba = rc_v(p.v + 3) - c;
        float s = xk::dot(x - c, ba) / xk::dot(ba, ba);
        s = fminf(fmaxf(s, 0.0f), 1.0f);
        n = x - (c + ba * s);
    }
    return n * (1.0f / sqrtf(xk::dot(n, n)));
}

XARM_HD uint32_t rc_pack(float r, float g, float b) {
    const uint32_t R = (uint32_t)(fminf(r, 1.0f) * 255.0f + 0.5f), G = (uint32_t)(fminf(g, 1.0f) * 255.0f + 0.5f),
                   B = (uint32_t)(fminf(b, 1.0f) * 255.0f + 0.5f);
    return R | (G << 8) | (B << 16) | (255u << 24);
}

XARM_HD V3<float> rc_ray(const RCam &cam, int i, int j) {
    const float x = (2.0f * ((float)j + 0.5f)) / (float)cam.width - 1.0f, y = 1.0f - (2.0f * ((float)i + 0.5f)) / (float)cam.height;
    return rc_v(cam.fwd) + rc_v(cam.right) * x + rc_v(cam.up) * y;
}

// pixel (i, j) (row 0 = top): primary ray over the primitives of `mask` (a superset of those it can hit: the kernel's tile
// culling, all of them in the host build), shadow ray over all nprim
XARM_HD void rc_pixel(const RPrim *P, int nprim, uint64_t mask, const RCam &cam, int i, int j, uint32_t &rgba, float &depth, uint8_t &seg) {
    const V3<float> o = rc_v(cam.eye), d = rc_ray(cam, i, j);
    float tb = cam.far_z;
    int hit = -1;
    while (mask) {
        const int k = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float t = rc_intersect(P[k], o, d, cam.near_z);
        if (t < tb) { tb = t; hit = k; }
    }
    if (hit < 0) {
        rgba = rc_pack(xrm::PALETTE[C_BACKGROUND][0], xrm::PALETTE[C_BACKGROUND][1], xrm::PALETTE[C_BACKGROUND][2]);
        depth = cam.far_z;
        seg = SEG_BACKGROUND;
        return;
    }
    const float m = P[hit].v[15];
    const V3<float> x = o + d * tb;
    V3<float> nrm = rc_normal(P[hit], x);
    if (xk::dot(nrm, d) > 0.0f) nrm = nrm * -1.0f;
    const V3<float> L = mk<float>(xrm::LIGHT_DIR[0], xrm::LIGHT_DIR[1], xrm::LIGHT_DIR[2]);
    float diff = fmaxf(xk::dot(nrm, L), 0.0f);
    if ((cam.flags & XARM_RENDER_SHADOWS) && diff > 0.0f) {
        const V3<float> so = x + nrm * 1e-3f;
        for (int k = 0; k < nprim; k++)
            if (rc_intersect(P[k], so, L, 0.0f) < RC_INF) { diff = 0.0f; break; }
    }
    const float s = xrm::AMBIENT + xrm::DIFFUSE * diff;
    const int pal = rc_pal(m);
    rgba = rc_pack(xrm::PALETTE[pal][0] * s, xrm::PALETTE[pal][1] * s, xrm::PALETTE[pal][2] * s);
    depth = tb;
    seg = (uint8_t)rc_seg(m);
}

// does the bounding sphere b reach into the frustum of the pixel rectangle rows [i0, i1) x columns [j0, j1)?  (conservative)
XARM_HD bool rc_bound_visible(const RBound &b, const RCam &cam, int i0, int i1, int j0, int j1) {
    if (b.c[3] < 0.0f) return true;
    const float r = b.c[3] * 1.001f + 1e-4f;
    const V3<float> rel = mk<float>(b.c[0] - cam.eye[0], b.c[1] - cam.eye[1], b.c[2] - cam.eye[2]);
    if (xk::dot(rel, rc_v(cam.fwd)) + r < cam.near_z) return false;
    const float xl = 2.0f * (float)j0 / (float)cam.width - 1.0f, xr = 2.0f * (float)j1 / (float)cam.width - 1.0f;
    const float yt = 1.0f - 2.0f * (float)i0 / (float)cam.height, yb = 1.0f - 2.0f * (float)i1 / (float)cam.height;
    const V3<float> F = rc_v(cam.fwd), R = rc_v(cam.right), U = rc_v(cam.up);
    const V3<float> tl = F + R * xl + U * yt, tr = F + R * xr + U * yt, bl = F + R * xl + U * yb, br = F + R * xr + U * yb;
    const V3<float> ctr = F + R * (0.5f * (xl + xr)) + U * (0.5f * (yt + yb));
    const V3<float> pairs[4][2] = {{tl, bl}, {br, tr}, {tr, tl}, {bl, br}};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        V3<float> n = xk::cross(pairs[k][0], pairs[k][1]);
        if (xk::dot(n, ctr) < 0.0f) n = n * -1.0f;
        if (xk::dot(n, rel) < -r * sqrtf(xk::dot(n, n))) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------- views
// A view record (include/xarm_hip.h XARM_VIEW_FLOATS = 16 float32, device-resident): eye [0..2], target [3..5], up [6..8] in
// the MOUNT's frame (PyBullet's computeViewMatrix arguments), fov_deg [9] (vertical), near_z [10], far_z [11], mount [12]
// (XARM_MOUNT_WORLD 0, XARM_MOUNT_HAND0 1, XARM_MOUNT_HAND1 2: the hand frame of arm 0 / 1); [13..15] ignored.
//
// VALIDITY RULE (decided here, per (env, view), because the host never sees the record).  A view is valid iff all of:
//   floats 0-12 are finite (and so are the world-frame target - eye and up they give);
//   mount is exactly 0, 1 or 2 and a hand mount names an arm the scene has (mount <= narms);
//   0 < fov_deg < 180;  0 < near_z < far_z < 1e30;  |target - eye| > 1e-6;  |up| > 1e-6;  |f x up / |up|| > 1e-6
//   (f the unit view direction: the view direction is not parallel to up).
// An invalid view renders the invalid image (rgba 0, depth 0, segmentation SEG_INVALID), as an env id out of range does.
//
// rc_make_view builds the camera of a valid record in float32: world eye / target / up through the mount frame, then
// f = (target - eye) / |.|, s = f x up / |.|, u = s x f, right = s tan(fov / 2) W / H, up = u tan(fov / 2) - RCam's ray and
// depth convention (the ray parameter is the view-axis depth, row 0 the top).  Returns false for an invalid record
// (`out` is then unspecified).  hands[a] = the hand frame of arm a (rc_hand_frame), a < narms.
XARM_HD bool rc_finite(float x) { return fabsf(x) < RC_INF; }
// |v| without overflow or underflow of the squares (any finite v)
XARM_HD float rc_norm(V3<float> v) {
    const float m = fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z)));
    if (!(m > 0.0f)) return 0.0f;
    const V3<float> w = v * (1.0f / m);
    return m * sqrtf(xk::dot(w, w));
}

XARM_HD bool rc_make_view(const float *view16, const Frame<float> *hands, int narms, int W, int H, int flags, RCam &out) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 13; k++) fin = fin && rc_finite(view16[k]);
    if (!fin) return false;
    const float fov = view16[9], near_z = view16[10], far_z = view16[11], m = view16[12];
    if (!(m == 0.0f || m == 1.0f || m == 2.0f)) return false;
    const int mount = (int)m;
    if (mount > narms) return false;
    if (!(fov > 0.0f && fov < 180.0f)) return false;
    if (!(near_z > 0.0f && far_z > near_z && far_z < 1e30f)) return false;
    Frame<float> F = xk::frame_identity<float>();
    if (mount != XARM_MOUNT_WORLD) F = hands[mount - 1];
    const V3<float> eye = F.o + F.c0 * view16[0] + F.c1 * view16[1] + F.c2 * view16[2];
    const V3<float> tgt = F.o + F.c0 * view16[3] + F.c1 * view16[4] + F.c2 * view16[5];
    const V3<float> up = F.c0 * view16[6] + F.c1 * view16[7] + F.c2 * view16[8];
    const V3<float> d = tgt - eye;
    if (!(rc_finite(d.x) && rc_finite(d.y) && rc_finite(d.z) && rc_finite(up.x) && rc_finite(up.y) && rc_finite(up.z))) return false;
    const float dl = rc_norm(d), ul = rc_norm(up);
    if (!(dl > 1e-6f && ul > 1e-6f)) return false;
    const V3<float> f = d * (1.0f / dl);
    V3<float> s = xk::cross(f, up * (1.0f / ul));
    const float sl = sqrtf(xk::dot(s, s));
    if (!(sl > 1e-6f)) return false;
    s = s * (1.0f / sl);
    const V3<float> u = xk::cross(s, f);
    const float ty = tanf(0.5f * fov * 0.017453292519943295f), tx = ty * (float)W / (float)H;
    out.eye[0] = eye.x; out.eye[1] = eye.y; out.eye[2] = eye.z;
    out.fwd[0] = f.x; out.fwd[1] = f.y; out.fwd[2] = f.z;
    out.right[0] = s.x * tx; out.right[1] = s.y * tx; out.right[2] = s.z * tx;
    out.up[0] = u.x * ty; out.up[1] = u.y * ty; out.up[2] = u.z * ty;
    out.near_z = near_z; out.far_z = far_z; out.width = W; out.height = H; out.flags = flags;
    return true;
}

// ---------------------------------------------------------------------------------------------------- host-side setup
// the scene layout of a handle's configuration; returns 0, or -1 for an unknown kind
inline int rc_scene_of(int kind, int num_obj, int use_stand, RScene &sc) {
    sc.kind = kind; sc.use_stand = 0;
    sc.goal_radius = (kind >= 0 && kind <= XARM_ENV_REARRANGE) ? xrm::GOAL_RADIUS[kind] : 0.0f;
    if (kind == XARM_ENV_PICK_AND_PLACE) {
        sc.narms = 1; sc.arm_prims = 10; sc.nobj = 1; sc.ngoal = 1; sc.nstatic = 2;
        sc.q_off = xk::S_Q; sc.bp_off = xk::S_BP; sc.bq_off = xk::S_BQ; sc.goal_off = xk::S_GOAL;
        for (int k = 0; k < 3; k++) sc.obj_half[k] = xrm::PNP_OBJ_HALF[k];
    } else if (kind == XARM_ENV_REACH) {
        sc.narms = 1; sc.arm_prims = 8; sc.nobj = 0; sc.ngoal = 1; sc.nstatic = 2;
        sc.q_off = xr::R_Q; sc.bp_off = 0; sc.bq_off = 0; sc.goal_off = xr::R_GOAL;
        for (int k = 0; k < 3; k++) sc.obj_half[k] = 0.0f;
    } else if (kind == XARM_ENV_HANDOVER) {
        const bool two = num_obj == 2;
        sc.narms = 2; sc.arm_prims = 10; sc.nobj = two ? 2 : 1; sc.ngoal = sc.nobj;
        sc.use_stand = use_stand ? 1 : 0; sc.nstatic = 3 + sc.use_stand;
        sc.q_off = two ? (int)xh2::G_Q : (int)xh::H_Q; sc.bp_off = two ? (int)xh2::G_BP : (int)xh::H_BP;
        sc.bq_off = two ? (int)xh2::G_BQ : (int)xh::H_BQ;
        sc.goal_off = two ? (int)xh2::G_GOAL : (int)xh::H_GOAL;
        for (int k = 0; k < 3; k++) sc.obj_half[k] = xrm::HO_OBJ_HALF[k];
    } else if (kind == XARM_ENV_STACK_TOWER) {
        sc.narms = 2; sc.arm_prims = 10; sc.nobj = 3; sc.ngoal = 3; sc.nstatic = 2;
        sc.q_off = xs::K_Q; sc.bp_off = xs::K_BP; sc.bq_off = xs::K_BQ; sc.goal_off = xs::K_GOAL;
        for (int k = 0; k < 3; k++) sc.obj_half[k] = xrm::ST_CUBE_HALF;
    } else if (kind == XARM_ENV_REARRANGE) {
        sc.narms = 2; sc.arm_prims = 10; sc.nobj = 4; sc.ngoal = 4; sc.nstatic = 2;
        sc.q_off = xra::K_Q; sc.bp_off = xra::K_BP; sc.bq_off = xra::K_BQ; sc.goal_off = xra::K_GOAL;
        for (int k = 0; k < 3; k++) sc.obj_half[k] = xrm::RA_CUBE_HALF;
    } else {
        return -1;
    }
    sc.nprim = sc.narms * sc.arm_prims + sc.nobj + sc.ngoal + sc.nstatic;
    return 0;
}

inline int rc_default_camera(int kind, xarm_camera &c) {
    if (kind < 0 || kind > XARM_ENV_REARRANGE) return -1;
    for (int k = 0; k < 3; k++) c.target[k] = xrm::CAM_TARGET[kind][k];
    c.distance = xrm::CAM_DISTANCE[kind]; c.yaw_deg = xrm::CAM_YAW[kind]; c.pitch_deg = xrm::CAM_PITCH[kind];
    c.roll_deg = xrm::CAM_ROLL[kind]; c.fov_deg = xrm::CAM_FOV[kind]; c.near_z = xrm::CAM_NEAR[kind]; c.far_z = xrm::CAM_FAR[kind];
    c.width = xrm::CAM_WIDTH[kind]; c.height = xrm::CAM_HEIGHT[kind]; c.flags = 0;
    return 0;
}

// eye and up of a camera: eye = M (0, -distance, 0) + target, up = M (0, 0, 1), M = Rz(yaw) Ry(roll) Rx(pitch)
inline void rc_camera_pose(const xarm_camera &c, double (&eye)[3], double (&up)[3]) {
    const double D = 3.14159265358979323846 / 180.0;
    const double cy = cos(c.yaw_deg * D), sy = sin(c.yaw_deg * D), cr = cos(c.roll_deg * D), sr = sin(c.roll_deg * D);
    const double cp = cos(c.pitch_deg * D), sp = sin(c.pitch_deg * D);
    const double Rz[3][3] = {{cy, -sy, 0}, {sy, cy, 0}, {0, 0, 1}}, Ry[3][3] = {{cr, 0, sr}, {0, 1, 0}, {-sr, 0, cr}},
                 Rx[3][3] = {{1, 0, 0}, {0, cp, -sp}, {0, sp, cp}};
    double A[3][3], M[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            A[i][j] = 0; for (int k = 0; k < 3; k++) A[i][j] += Rz[i][k] * Ry[k][j];
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            M[i][j] = 0; for (int k = 0; k < 3; k++) M[i][j] += A[i][k] * Rx[k][j];
        }
    for (int i = 0; i < 3; i++) { eye[i] = -c.distance * M[i][1] + c.target[i]; up[i] = M[i][2]; }
}

// PyBullet's computeViewMatrixFromYawPitchRoll (upAxisIndex 2) + computeProjectionMatrixFOV in closed form:
// eye = Rz(yaw) Ry(roll) Rx(pitch) (0, -distance, 0) + target, up = the same rotation of (0, 0, 1), then a look-at.
// Returns a message for an argument out of range, 0 when the camera is valid.
inline const char *rc_make_camera(const xarm_camera &c, RCam &out) {
    if (!(c.width >= 1 && c.width <= XARM_RENDER_MAX_DIM && c.height >= 1 && c.height <= XARM_RENDER_MAX_DIM))
        return "width and height must lie in [1, XARM_RENDER_MAX_DIM]";
    if (!(c.fov_deg > 0.0f && c.fov_deg < 180.0f)) return "fov_deg must lie in (0, 180)";
    if (!(c.near_z > 0.0f && c.far_z > c.near_z && c.far_z < 1e30f)) return "need 0 < near_z < far_z < 1e30";
    if (!(c.distance > 0.0f && c.distance < 1e30f)) return "distance must be positive";
    if (c.flags & ~XARM_RENDER_SHADOWS) return "unknown flag bits";
    for (int k = 0; k < 3; k++)
        if (!(fabsf(c.target[k]) < 1e30f)) return "target must be finite";
    if (!(fabsf(c.yaw_deg) < 1e6f && fabsf(c.pitch_deg) < 1e6f && fabsf(c.roll_deg) < 1e6f)) return "angles must be finite";
    const double D = 3.14159265358979323846 / 180.0;
    double eye[3], up[3], f[3], s[3], u[3];
    rc_camera_pose(c, eye, up);
    for (int i = 0; i < 3; i++) f[i] = c.target[i] - eye[i];
    double fn = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (int i = 0; i < 3; i++) f[i] /= fn;
    s[0] = f[1] * up[2] - f[2] * up[1]; s[1] = f[2] * up[0] - f[0] * up[2]; s[2] = f[0] * up[1] - f[1] * up[0];
    const double sn = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (!(sn > 1e-9)) return "view direction parallel to the up vector";
    for (int i = 0; i < 3; i++) s[i] /= sn;
    u[0] = s[1] * f[2] - s[2] * f[1]; u[1] = s[2] * f[0] - s[0] * f[2]; u[2] = s[0] * f[1] - s[1] * f[0];
    const double ty = tan(0.5 * c.fov_deg * D), tx = ty * (double)c.width / (double)c.height;
    for (int i = 0; i < 3; i++) {
        out.eye[i] = (float)eye[i]; out.fwd[i] = (float)f[i]; out.right[i] = (float)(s[i] * tx); out.up[i] = (float)(u[i] * ty);
    }
    out.near_z = c.near_z; out.far_z = c.far_z; out.width = c.width; out.height = c.height; out.flags = c.flags;
    return 0;
}

// the view record of a camera: mount WORLD, the eye / target / up rc_make_camera looks along, its fov and clip planes (the
// image size and the flags are arguments of the render call, not of the view).  Returns a message for an argument out of
// range, 0 when the record was written.
inline const char *rc_view_from_camera(const xarm_camera &c, float (&out)[XARM_VIEW_FLOATS]) {
    xarm_camera probe = c;
    probe.width = probe.height = 1; probe.flags = 0;
    RCam rc;
    if (const char *why = rc_make_camera(probe, rc)) return why;
    double eye[3], up[3];
    rc_camera_pose(c, eye, up);
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) out[k] = 0.0f;
    for (int k = 0; k < 3; k++) { out[k] = (float)eye[k]; out[3 + k] = c.target[k]; out[6 + k] = (float)up[k]; }
    out[9] = c.fov_deg; out[10] = c.near_z; out[11] = c.far_z; out[12] = (float)XARM_MOUNT_WORLD;
    return 0;
}

// the default views of an env kind: which = 0 the default camera as a world view, 1 / 2 the wrist view of arm 0 / 1
// (render_scene.json "views").  Returns 0, or -1 for an unknown kind / which or an arm the kind does not have.
inline int rc_default_view(int kind, int which, float (&out)[XARM_VIEW_FLOATS]) {
    RScene sc;
    if (rc_scene_of(kind, 1, 0, sc) != 0 || which < 0 || which > sc.narms) return -1;
    if (which == 0) {
        xarm_camera c;
        if (rc_default_camera(kind, c) != 0) return -1;
        return rc_view_from_camera(c, out) ? -1 : 0;
    }
    for (int k = 0; k < XARM_VIEW_FLOATS; k++) out[k] = 0.0f;
    for (int k = 0; k < 3; k++) { out[k] = xrm::WRIST_EYE[k]; out[3 + k] = xrm::WRIST_TARGET[k]; out[6 + k] = xrm::WRIST_UP[k]; }
    out[9] = xrm::WRIST_FOV; out[10] = xrm::WRIST_NEAR; out[11] = xrm::WRIST_FAR;
    out[12] = (float)(which == 1 ? XARM_MOUNT_HAND0 : XARM_MOUNT_HAND1);
    return 0;
}

#if defined(__HIPCC__) && !defined(XARM_HOST_BUILD)
// k_render over the n envs ids[0 .. n) (null: 0 .. n-1) on `stream` (xarm_k_render.hip); returns the launch's hipError_t
int launch_render(const float *state, int64_t stride, int64_t num_envs, const RScene &sc, const RCam &cam, const int32_t *ids, int32_t n,
                  uint32_t *rgba, float *depth, uint8_t *seg, void *stream);
// k_render_views: the V views views[(per_env ? k * V : 0) + v] of each env ids[k], into [n, V, height, width] outputs
int launch_render_views(const float *state, int64_t stride, int64_t num_envs, const RScene &sc, const float *views, int32_t num_views,
                        int32_t per_env, int32_t width, int32_t height, int32_t flags, const int32_t *ids, int32_t n, uint32_t *rgba,
                        float *depth, uint8_t *seg, void *stream);
#endif

}  // namespace xrc_render
