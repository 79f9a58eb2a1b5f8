// XarmRearrange-v0 on the device: StackTower's two xarm7_pd arms (one lane each) and FOUR cubes, each with its own goal.
//
// Reference: gym_xarm/envs/xarm_rearrange.py (XarmRearrangeEnv; xarm_bimanual_base.py XarmPDBimanualEnv is the
// same file but for the class name).  It differs from xarm_stack_tower.py in num_obj = 4 (:20, so distance_threshold 0.12) and
// _sample_goal (:213-218: an independent goal_space xy per cube at z = 0.025) only.  Arms, clip boxes, gripper range, cubes,
// the reset (one tick, no rejection), done = False, 50 steps and the contact model are StackTower's: the scene is the cube
// core of xarm_stack_core.h (state and observation layout, row order, class key, LDS columns: its header comment) with
// N = 4 - six cube pairs, 256 row-set classes, STATE_DIM 160, OBS_DIM 68 - plus the goal sampling below.
// Draws: blocks 0-1 = u[0..7] = cube i xy - cubes 0-2 spawn where StackTower's do; blocks 2-3 = u[8..15] = goal i xy
// (u[8+2i], u[9+2i]).
#pragma once
#include "xarm_stack_core.h"

namespace xra {

struct Rearrange4 : xs::Cubes<4> {
    static constexpr double OBJ_LOW[2] = {xm::RA_OBJ_LOW[0], xm::RA_OBJ_LOW[1]}, OBJ_HIGH[2] = {xm::RA_OBJ_HIGH[0], xm::RA_OBJ_HIGH[1]};
    static constexpr double DISTANCE_THRESHOLD = xm::RA_DISTANCE_THRESHOLD;
    static constexpr int MAX_EPISODE_STEPS = xm::RA_MAX_EPISODE_STEPS;
    static constexpr int NDRAW = 16;
    template <typename T> static XARM_HD void sample_goal(const T (&u)[NDRAW], xs::Lane<T, Rearrange4> &L) {
#pragma unroll
        for (int o = 0; o < NOBJ; o++) {   // :213-218: one goal_space xy per cube, on the table
            L.goal[o][0] = (T)xm::RA_GOAL_LOW[0] + u[8 + 2 * o] * (T)(xm::RA_GOAL_HIGH[0] - xm::RA_GOAL_LOW[0]);
            L.goal[o][1] = (T)xm::RA_GOAL_LOW[1] + u[9 + 2 * o] * (T)(xm::RA_GOAL_HIGH[1] - xm::RA_GOAL_LOW[1]);
            L.goal[o][2] = (T)xm::ST_HEIGHT_OFFSET;
        }
    }
};
static_assert(xm::RA_NUM_OBJ == Rearrange4::NOBJ, "model JSON rearrange.num_obj");
static_assert(Rearrange4::K_BQ == 66 && Rearrange4::K_BV == 82 && Rearrange4::K_BW == 94 && Rearrange4::K_GOAL == 106 && Rearrange4::K_LT == 118 &&
              Rearrange4::K_LP == 150 && Rearrange4::K_STEPS == 158 && Rearrange4::K_EPISODE == 159, "Rearrange state layout");
static_assert(Rearrange4::STATE_DIM == 160 && Rearrange4::OBS_DIM == 68 && Rearrange4::GOAL_DIM == 12 && Rearrange4::NCLS == 256, "Rearrange sizes");
static_assert(Rearrange4::LDS_FLOATS == 929 && Rearrange4::LDS_SHARED == 812, "DESIGN.md 17 LDS arithmetic");
static_assert(Rearrange4::pair_a(2) == 0 && Rearrange4::pair_b(2) == 3 && Rearrange4::pair_a(3) == 1 && Rearrange4::pair_b(3) == 2 &&
              Rearrange4::pair_a(4) == 1 && Rearrange4::pair_b(4) == 3 && Rearrange4::pair_a(5) == 2 && Rearrange4::pair_b(5) == 3, "pairs 01 02 03 12 13 23");

// the namespace-level names, and the core's entry points under this namespace (the scene is deduced from the Lane)
XARM_CUBE_SCENE_NAMES(Rearrange4);
template <typename T> using Lane = xs::Lane<T, Rearrange4>;
using xs::lane_init; using xs::lane_step; using xs::lane_reset; using xs::arm_obs; using xs::class_layout; using xs::class_slot;

} // namespace xra
