/*
 * xarm_hip.h - C ABI of libxarm_hip.so, the MI355X (gfx950) batched Xarm7 manipulation
 * environment.  This is the drop-in boundary for the hot path of jc-bao/gym-xarm:
 *
 *   reference interface (Python, /root/reference/gym_xarm/envs/xarm_pick_and_place.py)
 *     XarmPickAndPlace.__init__(config)            :17-103   -> xarm_create
 *     XarmPickAndPlace.reset()                     :121-127  -> xarm_reset
 *     XarmPickAndPlace.step(action)                :107-119  -> xarm_step
 *     XarmPickAndPlace.compute_reward(ag, g, info) :155-177  -> xarm_compute_reward
 *     XarmPickAndPlace.close / p.disconnect                  -> xarm_destroy
 *   and the PyBullet C-API calls those methods make per step, which this
 *   library replaces wholesale:  calculateInverseKinematics :207, setJointMotorControl2
 *   :208-211, getContactPoints :212, changeDynamics :213-218, stepSimulation :111,
 *   getLinkState/getJointStates/getBasePositionAndOrientation/getBaseVelocity :222-236.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative
 *     XARM_E_* code and never throws; xarm_last_error() gives the message.
 *   - all *_dev pointers are DEVICE pointers borrowed from the caller (e.g. torch tensors'
 *     data_ptr()), row-major [num_envs, dim], float32 unless stated; they must stay valid
 *     until the stream has executed the call.
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls are
 *     asynchronous, the caller synchronises.
 *   - one handle per GPU per process; a handle is not thread-safe.
 */
#ifndef XARM_HIP_H
#define XARM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XARM_OK 0
#define XARM_E_INVALID (-1)   /* bad argument / unsupported configuration */
#define XARM_E_HIP (-2)       /* a HIP runtime call failed */
#define XARM_E_NODEVICE (-3)  /* no HIP device available */

#define XARM_ENV_PICK_AND_PLACE 0 /* XarmPickAndPlace-v1 / XarmPDPickAndPlace-v0 (xarm_pick_and_place.py) */
#define XARM_ENV_REACH 1          /* XarmReach-v0 (xarm_reach.py): obs 8, 25 steps, 20 substeps of 1/4800 s;
                                     xarm_config.num_obj / goal_shape / *_rate are ignored */
#define XARM_ENV_HANDOVER 2       /* XarmHandover-v0 / XarmPDHandover-v0 (xarm_handover.py): two arms, one stick,
                                     obs 29, action 8, sparse reward -1/0, 100 steps; uses same_side_rate and
                                     goal_shape (XARM_GOAL_GROUND = 'ground', else the sampled height) */
#define XARM_ENV_STACK_TOWER 3    /* XarmPDStackTower-v0 (xarm_stack_tower.py): two arms, three cubes (num_obj = 3),
                                     obs 55, action 8, goal 9, reward_type 0 = -(d > 0.09) / 1 = -d (:124-129),
                                     50 steps (:43); step() itself never reports done (:111) */
#define XARM_ENV_REARRANGE 4      /* XarmRearrange-v0 (xarm_rearrange.py): StackTower's two arms with four cubes (num_obj = 4)
                                     and one goal per cube; obs 68, action 8, goal 12, reward_type 0 = -(d > 0.12) /
                                     1 = -d over the 12-vector, 50 steps; step() never reports done; goal_shape and the
                                     *_rate fields are ignored, use_stand and XARM_AUTO_RESET_LAZY are refused */

/* auto_reset = XARM_AUTO_RESET_LAZY (PickAndPlace only; NOT the reference's semantics, opt-in for throughput): an env that
 * finishes an episode runs the reference's six reset ticks (xarm_pick_and_place.py:250-266) one per call in its next six
 * xarm_step calls instead of inside the call in which it finished.  The tick sequence, and so the state the new episode
 * starts from, is the same.  done[e] then reports the phase: 0 ordinary step, 1 the episode ended in this call (obs =
 * terminal observation), 2 reset tick (action ignored, reward 0, to be masked by the learner; the sixth such call returns
 * the first observation of the new episode).  No terminal_obs buffer is written. */
#define XARM_AUTO_RESET_LAZY 2

#define XARM_REWARD_SPARSE 0    /* (|ag-g| < 0.05) -> 1/0            :163-165 */
#define XARM_REWARD_DENSE_O2G 1 /* -|ag-g|                           :176-177 */
#define XARM_REWARD_DENSE 2     /* staged reach/grasp/lift reward    :166-175; uses the simulator's contact
                                   state, so xarm_compute_reward (relabelling) rejects it */

/* XarmReach-v0 reward types, xarm_reach.py:107-116 */
#define XARM_REACH_REWARD_SPARSE 0     /* (|ag-g| < 0.05) -> 1/0 */
#define XARM_REACH_REWARD_DENSE 1      /* -|ag-g| */
#define XARM_REACH_REWARD_DENSE_DIFF 2 /* d_old - d, stateful: xarm_compute_reward rejects it */

#define XARM_GOAL_AIR 0    /* goal_space.sample(), z -> ground w.p. goal_ground_rate  :272-280 */
#define XARM_GOAL_GROUND 1 /* shared xy, z = 0.025 (2i+1)                             :282-286 */

typedef struct xarm_config {
    int64_t num_envs;       /* environments owned by this handle (this GPU's shard) */
    int64_t env_id_offset;  /* global id of env 0 of the shard; the RNG is keyed by global id */
    uint64_t seed;
    int32_t env_kind;       /* XARM_ENV_* */
    int32_t num_obj;        /* config['num_obj']: 1; XarmHandover also 2 (the reference's test.py:9-15: obs 42, goals 6); StackTower 3; Rearrange 4 */
    int32_t reward_type;    /* XARM_REWARD_* (config['reward_type']) */
    int32_t goal_shape;     /* XARM_GOAL_*   (config['goal_shape']) */
    float init_grasp_rate;  /* config['init_grasp_rate'] */
    float goal_ground_rate; /* config['goal_ground_rate'] */
    int32_t auto_reset;     /* 1: envs that finish an episode in xarm_step are reset in the same call (the reference's
                               VecEnv semantics); XARM_AUTO_RESET_LAZY: see below */
    int32_t device;         /* HIP device ordinal */
    float same_side_rate;   /* config['same_side_rate'] (Handover, xarm_handover.py:380) */
    int32_t reset_coop_limit; /* PickAndPlace, Reach, Handover (one stick): resets of at most this many envs per call run on the cooperative
                               (16 lanes per env) kernel; 0 = default (XARM_RESET_COOP_LIMIT_DEFAULT), < 0 = never */
    int32_t step_coop_limit;  /* PickAndPlace, Reach, Handover (one stick): a handle of at most this many envs also STEPS on the cooperative kernel
                                 (the one-env-per-lane launch would leave most SIMDs without a wavefront);
                                 0 = default (XARM_STEP_COOP_LIMIT_DEFAULT), < 0 = never.  Larger PickAndPlace handles step on
                                 the pad-free fast kernel and hand the envs with an active finger-pad row to the cooperative
                                 kernel (XARM_EJECT_COOP_CAP); < 0 also pins those to the plain one-env-per-lane k_step */
    int32_t use_stand;        /* XarmHandover config['use_stand'] (xarm_handover.py:391-392): a static 0.07 x 0.06 x 0.01 box
                                 whose top sits 25 mm under the goal; 0 = parked away (the BASELINE configuration) */
} xarm_config;                /* 72 bytes */
#define XARM_RESET_COOP_LIMIT_DEFAULT 8192
/* PickAndPlace batches above step_coop_limit step on the pad-free fast kernel; the envs with an active finger-pad row
 * (~2 % in the steady state, ~16 % in the first steps after a bulk reset) are handed off to the cooperative kernel -
 * hand-offs of more than this many envs to the one-env-per-lane kernel.  The break-even is ~8 192 envs; the cap is set
 * well above it (the first steps after a bulk reset of 65 536 envs hand off ~17 000) so that the choice - which, like the
 * reset family, depends on a COUNT and therefore on the shard - is only ever crossed by configurations that start most
 * episodes in the gripper (init_grasp_rate) */
#define XARM_EJECT_COOP_CAP 32768
/* A pipelined step with auto-reset resets the episodes that ended in the fast kernel on a side stream owned by the handle,
 * in parallel with the hand-off, and joins it (event wait) before its work on the caller's stream ends: the caller sees one
 * stream-ordered call.  XARM_RESET_OVERLAP=0 in the environment at xarm_create keeps everything on the caller's stream.
 * The episodes that end in a hand-off kernel: with XARM_RESET_PER_STAGE_DEFAULT (env XARM_RESET_PER_STAGE = 0 / 1 at xarm_create)
 * every hand-off stage of a staged step keeps a list of its own and resets it directly behind its hand-off, on that stage's side
 * stream (the last stage's on the caller's stream); without, one list for all stages is reset after the last hand-off.  Same
 * results either way: an env's reset does not depend on the envs it shares a wavefront with. */
#define XARM_RESET_PER_STAGE_DEFAULT 1
/* PickAndPlace handles of at most this many envs step on the cooperative kernel as well (env XARM_STEP_COOP_LIMIT) */
#define XARM_STEP_COOP_LIMIT_DEFAULT 8192
/* XarmHandover with one stick steps the same way at every batch size (unless step_coop_limit < 0 or XARM_STEP_PIPELINE=0 select
 * the plain lane-pair k_ho_step): the pad-free fast lane-pair kernel, then the envs with an active finger-pad row on either arm
 * (~4 %) on the cooperative rows - TWO 16-lane rows per env, one per arm (csrc/xarm_handover_coop_core.h).  Hand-offs of more
 * than XARM_HO_EJECT_COOP_CAP envs go to k_ho_step instead (2 048 cooperative wavefronts per round of ~0.5 ms against 2.3 ms);
 * resets of at most XARM_HO_RESET_COOP_LIMIT_DEFAULT envs (reset_coop_limit / XARM_RESET_COOP_LIMIT override) run on the
 * cooperative rows too. */
#define XARM_HO_EJECT_COOP_CAP 8192
#define XARM_HO_RESET_COOP_LIMIT_DEFAULT 4096
/* ... and a Handover handle of at most XARM_HO_STEP_COOP_LIMIT_DEFAULT envs (step_coop_limit / XARM_STEP_COOP_LIMIT override, as
 * for PickAndPlace) steps on the cooperative rows altogether: one launch, no fast pass */
#define XARM_HO_STEP_COOP_LIMIT_DEFAULT 2048
/* The Handover pipeline is STAGED: the fast kernel runs the 15 ticks of a step in XARM_HO_STAGES_DEFAULT launches (env
 * XARM_HO_STAGES = 1 .. 5 at xarm_create; 1 = one fast launch and one hand-off).  An env whose pads come alive in stage c keeps the
 * state it had before that stage and re-runs the ticks from the stage's first one on the cooperative rows, on a side stream
 * owned by the handle, beside the next fast stage; every side stream is joined (event wait) before the call's work on the
 * caller's stream ends.  Which kernel runs which tick of an env is a function of that env's own state and of the handle's
 * configuration, never of its neighbours. */
#define XARM_HO_STAGES_DEFAULT 3
/* The pipelined PickAndPlace step (batches above step_coop_limit) is staged the same way over its 15 substeps: XARM_PNP_STAGES_DEFAULT
 * fast launches (env XARM_PNP_STAGES = 1 .. 5 at xarm_create; 1 = one fast launch and one hand-off: the unstaged pipeline, which is
 * the single stage {0, 15} of the same kernels, as XARM_HO_STAGES=1 is for Handover). */
#define XARM_PNP_STAGES_DEFAULT 3
/* test hook: XARM_HO_FORCE_COUPLED=1 at xarm_create sends every substep of the cooperative Handover step and reset through the
 * coupled (both-arms) sweep - same bits by construction (tests/test_handover_coop.py) */

typedef struct xarm_dims_t {
    int32_t obs_dim, goal_dim, act_dim, state_dim, max_episode_steps, n_substeps;
} xarm_dims_t;

typedef struct xarm_handle xarm_handle;

int xarm_create(const xarm_config *cfg, xarm_handle **out);
int xarm_destroy(xarm_handle *h);
int xarm_dims(const xarm_handle *h, xarm_dims_t *out);

/* reset(): mask_dev (uint8 [E], nullable = all envs) selects the environments to reset; the fresh
 * observation rows of those envs are written, other rows are left untouched. */
int xarm_reset(xarm_handle *h, const uint8_t *mask_dev, float *obs_dev, float *achieved_goal_dev,
               float *desired_goal_dev, void *stream);

/* step(actions): actions [E,4]; outputs obs [E,24], achieved/desired goal [E,3], reward [E],
 * done / is_success uint8 [E].  With auto_reset, rows of finished envs hold the first observation
 * of the next episode and terminal_obs_dev (nullable, [E,24]) receives their last observation. */
int xarm_step(xarm_handle *h, const float *actions_dev, float *obs_dev, float *achieved_goal_dev,
              float *desired_goal_dev, float *reward_dev, uint8_t *done_dev, uint8_t *success_dev,
              float *terminal_obs_dev, void *stream);

/* compute_reward(achieved_goal, goal, info) over n rows of goal_dim floats (HER relabelling) */
int xarm_compute_reward(xarm_handle *h, const float *achieved_goal_dev, const float *goal_dev, int64_t n,
                        float *out_dev, void *stream);

/* full simulator state, row-major [E, state_dim] (layout: gym_xarm_amd/csrc/xarm_core.h S_*);
 * used for parity injection and snapshots */
int xarm_get_state(xarm_handle *h, float *state_dev, void *stream);
int xarm_set_state(xarm_handle *h, const float *state_dev, void *stream);

/* steps taken in the current episode, int32 [E]; XarmReachEnv's info['future_length'] (xarm_reach.py:90) is
 * max_episode_steps - steps */
int xarm_episode_steps(xarm_handle *h, int32_t *steps_dev, void *stream);

/* test hook: advance every env by n internal substeps (dt = 1/900 s) toward the joint targets
 * qtarget_dev [E,9]; no action / IK / observation logic.  Used by the substep-level parity tests. */
int xarm_debug_substeps(xarm_handle *h, const float *qtarget_dev, int32_t n, void *stream);

/* optional kernel timing: HIP events recorded around the step kernel on the caller's stream */
int xarm_timing_enable(xarm_handle *h, int32_t enable);
int xarm_timing_read(xarm_handle *h, double *step_kernel_ms_total, int64_t *launches);
/* same for what follows the step kernel(s) on the caller's stream inside xarm_step (auto_reset): the reset kernels - and,
 * for a pipelined PickAndPlace call, only what is LEFT of them after the hand-off (the first reset launch runs on the
 * handle's side stream beside the hand-off; the join is inside this bracket).  Total ms over `launches` calls */
int xarm_timing_read_reset(xarm_handle *h, double *reset_kernels_ms_total, int64_t *launches);

/* the limits in force for this handle.  Precedence: an explicit xarm_config value (> 0, or < 0 = never) wins; with the
 * field at 0 the XARM_RESET_COOP_LIMIT / XARM_STEP_COOP_LIMIT environment variable replaces the built-in default: batches / reset lists of at most that many envs run on the cooperative kernels (0: never) */
int xarm_kernel_limits(const xarm_handle *h, int32_t *reset_coop_limit, int32_t *step_coop_limit);

/* which launches an xarm_step call of this handle is made of (what bench.py names the kernels from, instead of re-deriving it
 * from environment variables) and the solver constants the library was BUILT with:
 *   fast_pipeline    1: the pad-free fast step + the hand-off of the envs with an active finger-pad row to the cooperative
 *                    kernel (PickAndPlace batches above step_coop_limit, XarmHandover with one stick at every batch size);
 *                    0: one step kernel (the cooperative one for batches of at most step_coop_limit envs).  Only
 *                    step_coop_limit < 0 or XARM_STEP_PIPELINE=0 turn the pipeline off - XARM_STEP_COOP_LIMIT=0 turns off
 *                    the cooperative STEP kernel of small batches, not the pipeline of large ones
 *   reset_overlap    non-zero: PickAndPlace pipeline with the first reset launch on the handle's side stream (XARM_RESET_OVERLAP);
 *                    2: and a reset per hand-off stage behind that stage's hand-off (XARM_RESET_PER_STAGE), 1: one after the last
 *   eject_coop_cap   hand-off lists of at most this many envs step on the cooperative kernel, longer ones on the
 *                    one-env-per-lane kernel; INT32_MAX when step_coop_limit == 1 (the pin of
 *                    gym_xarm_amd.distributed.reproducible_limits('fast'): the choice is then a function of the config alone)
 *   solver_iterations  Gauss-Seidel sweeps per substep compiled into the kernels (50 = Bullet's numSolverIterations; a
 *                    timing variant built with -DXC_SWEEP_ITERS / -DXK_SWEEP_ITERS reports its own value and
 *                    xarm_version() says "TIMING VARIANT") */
int xarm_pipeline_info(const xarm_handle *h, int32_t *fast_pipeline, int32_t *reset_overlap, int32_t *eject_coop_cap,
                       int32_t *solver_iterations);
/* The stages of the staged Handover step (XARM_HO_STAGES_DEFAULT above): *stages = their number (1 for a handle without the
 * staged pipeline), ticks[0 .. *stages] = the first tick of each stage and, last, the tick count of a step; ticks has room for
 * XARM_HO_MAX_STAGES + 1 entries */
#define XARM_HO_MAX_STAGES 5
int xarm_stage_info(const xarm_handle *h, int32_t *stages, int32_t *ticks);
/* development / test hook: the device-side counters of the LAST xarm_step call, after synchronising `stream` - episodes that
 * ended in the step kernels (a pipelined PickAndPlace call counts the ones that ended in the hand-off apart: not included) and
 * envs handed off by the fast kernel to the cooperative one (0 for a handle without the pipeline; the staged Handover step: all stages) */
int xarm_debug_counts(xarm_handle *h, int32_t *finished, int32_t *handed_off, void *stream);
/* the same counters per stage of a pipelined step, arrays of XARM_HO_MAX_STAGES entries: handed_off[c] = envs handed off by fast
 * stage c, finished_in_handoff[c] = episodes that ended in the hand-off kernels of stage c (PickAndPlace with the side-stream reset;
 * without XARM_RESET_PER_STAGE entry 0 holds the count of all stages).  Zero for stages the handle does not have. */
int xarm_debug_stage_counts(xarm_handle *h, int32_t *handed_off, int32_t *finished_in_handoff, void *stream);

/* StackTower: the row-set class each env's last substep fell into, uint8 [E] (bits 0-2 cube pairs (0,1) (0,2) (1,2) in
 * contact, bit 3 / 4 a finger pad of arm 0 / 1 active).  The step
 * kernel visits the envs grouped by this key so that a wavefront sweeps one class's rows, not the union of 32 unrelated
 * envs' (csrc/xarm_stack_core.h "class-homogeneous wavefronts"); an env's result does not depend on the order.
 * XARM_ST_CLASS_ORDER=0 in the environment at xarm_create keeps the arrival order (then, and for the other env kinds,
 * this call fails with XARM_E_INVALID).  Rearrange: the same with bits 0-5 cube pairs 01 02 03 12 13 23, bit 6 / 7 a finger
 * pad of arm 0 / 1 (the same core with four cubes), switched off by XARM_RA_CLASS_ORDER=0.  Introspection only - nothing in
 * the reference corresponds to it. */
int xarm_class_keys(xarm_handle *h, uint8_t *keys_dev, void *stream);

/* ---- batched on-device rendering (gym_xarm_amd/csrc/xarm_render_core.h, xarm_k_render.hip).
 * Camera: PyBullet's computeViewMatrixFromYawPitchRoll (upAxisIndex 2) + computeProjectionMatrixFOV (vertical fov, aspect
 * width / height) restated in closed form; one ray through each pixel centre, row 0 = the top of the image.  The scene is
 * drawn from primitives (render_scene.json), not the reference's meshes: pixel parity with PyBullet is UNPINNED. */
#define XARM_RENDER_SHADOWS 1      /* xarm_camera.flags: one shadow ray per lit pixel */
#define XARM_RENDER_MAX_DIM 2048   /* width, height <= this */
typedef struct xarm_camera {
    float target[3], distance, yaw_deg, pitch_deg, roll_deg, fov_deg, near_z, far_z;
    int32_t width, height, flags;          /* XARM_RENDER_SHADOWS */
} xarm_camera;                             /* 52 bytes */
/* the env kind's default camera: PickAndPlace and Handover the reference's render() cameras, Reach / StackTower / Rearrange
 * build-defined (Rearrange = StackTower's: the reference sets the same debug camera in both scenes) */
int xarm_default_camera(const xarm_handle *h, xarm_camera *out);
/* render the n envs env_ids_dev[0 .. n) (int32 device array; NULL = envs 0 .. n-1) into rgba_dev (uint32 [n, height, width],
 * bytes R G B A, alpha 255), and, when not NULL, depth_dev (float32 [n, height, width]: view-axis eye-space distance in
 * metres, far_z for the background - NOT PyBullet's nonlinear z-buffer) and seg_dev (uint8 [n, height, width]: 0 background,
 * 1 table / ground / stand, 2 / 3 arm 0 links / gripper, 4 / 5 arm 1 links / gripper, 8 + k object k, 16 + k goal marker k).
 * Stream-ordered, never synchronises the host, reads the state the last xarm_step / xarm_reset on the stream left and writes
 * none of it; one kernel launch, no workspace (safe inside graph capture).  With auto_reset an env that finished in the last
 * step shows its NEW episode; with XARM_AUTO_RESET_LAZY it shows its terminal frame until its next xarm_step.  An env id
 * outside [0, num_envs) renders an all-zero image (rgba 0, depth 0) with segmentation 255.  XARM_E_INVALID: cam or rgba_dev
 * NULL, width / height outside [1, XARM_RENDER_MAX_DIM], n < 1 or n > num_envs, fov_deg outside (0, 180), not
 * 0 < near_z < far_z, distance <= 0, unknown flags. */
int xarm_render(xarm_handle *h, const xarm_camera *cam, const int32_t *env_ids_dev /* NULL = 0..n-1 */, int32_t n,
                uint32_t *rgba_dev, float *depth_dev /* may be NULL */, uint8_t *seg_dev /* may be NULL */, void *stream);

/* ---- views: link-mounted and per-env cameras, V views per call (k_render_views in xarm_k_render.hip).
 * A view is XARM_VIEW_FLOATS float32 in DEVICE memory, so that it can differ per env and change between the replays of a
 * captured graph:
 *   [0..2] eye, [3..5] target, [6..8] up - in the MOUNT's frame (PyBullet's computeViewMatrix arguments);
 *   [9] fov_deg (vertical), [10] near_z, [11] far_z, [12] mount, [13..15] ignored.
 * mount is a small integer stored exactly in the float: XARM_MOUNT_WORLD, or XARM_MOUNT_HAND0 / XARM_MOUNT_HAND1 = the hand
 * frame of arm 0 / 1 (the link-7 frame the arm's FK ends with: +z points to the fingertips, the fingers slide along y; for
 * Reach the same link-7 frame under the xArm gripper box).  The camera basis is built in the kernel in float32: world eye /
 * target / up through the mount frame, f = (target - eye) / |.|, s = f x up / |.|, u = s x f; rays, depth and row order as
 * xarm_render's.
 * VALIDITY RULE - the host never sees a record, so it is decided per (env, view) on the device.  A view is valid iff all of:
 *   floats 0-12 are finite (and so are the world-frame target - eye and up they give);  mount is exactly 0, 1 or 2 and a
 *   hand mount names an arm the scene has;  0 < fov_deg < 180;  0 < near_z < far_z < 1e30;  |target - eye| > 1e-6;
 *   |up| > 1e-6;  |f x up / |up|| > 1e-6 (the view direction is not parallel to up).
 * An invalid view renders the invalid image (rgba 0, depth 0, segmentation 255), exactly as an env id out of range does;
 * the call still returns XARM_OK and the other (env, view) images are unaffected. */
#define XARM_VIEW_FLOATS 16
#define XARM_RENDER_MAX_VIEWS 8
#define XARM_MOUNT_WORLD 0
#define XARM_MOUNT_HAND0 1
#define XARM_MOUNT_HAND1 2
/* host helpers, both write XARM_VIEW_FLOATS floats of HOST memory.  The world view with the eye / target / up, fov and clip
 * planes of a camera (its width / height / flags are arguments of the render call instead); XARM_E_INVALID for a camera
 * xarm_render would refuse on those fields. */
int xarm_view_from_camera(const xarm_camera *cam, float *view16_host);
/* which = 0: the env kind's default camera as a world view; 1 / 2: the default wrist view (render_scene.json "views") on
 * the hand of arm 0 / 1.  XARM_E_INVALID for which outside [0, 2] and for which = 2 on a one-arm kind. */
int xarm_default_view(const xarm_handle *h, int32_t which, float *view16_host);
/* xarm_render through num_views views per env in one launch: env env_ids_dev[k] (NULL = env k) through view v lands in
 * image [k, v] of rgba_dev (uint32 [n, num_views, height, width]) and, when not NULL, depth_dev (float32) / seg_dev (uint8)
 * of the same shape.  views_dev is float32 [num_views, 16] when per_env == 0 (shared by all envs) and [n, num_views, 16]
 * when per_env == 1, indexed by the POSITION k in the id list, the order of the output.  flags: XARM_RENDER_SHADOWS.
 * Stream-ordered, never synchronises the host, one kernel launch, no workspace (safe inside graph capture; the views are
 * read when the kernel runs), reads the state and writes none of it.  XARM_E_INVALID: views_dev or rgba_dev NULL, num_views
 * outside [1, XARM_RENDER_MAX_VIEWS], per_env not 0 or 1, width / height outside [1, XARM_RENDER_MAX_DIM], n < 1 or
 * n > num_envs, unknown flags. */
int xarm_render_views(xarm_handle *h, const float *views_dev, int32_t num_views, int32_t per_env, int32_t width, int32_t height,
                      int32_t flags, const int32_t *env_ids_dev /* NULL = 0..n-1 */, int32_t n, uint32_t *rgba_dev,
                      float *depth_dev /* may be NULL */, uint8_t *seg_dev /* may be NULL */, void *stream);

/* ---- device-resident hindsight-experience replay (gym_xarm_amd/csrc/xarm_her_core.h, xarm_k_her.hip).
 * The three calls need no env handle: the buffer is caller-owned DEVICE memory described by an xarm_her_layout, and the
 * launches go to `stream` on the caller's current device.  Messages of their XARM_E_INVALID go to xarm_last_error(NULL).
 *   ring      float32 [horizon, num_envs, R], one record per (slot, env):
 *             obs | next_obs | achieved_goal | next_achieved_goal | desired_goal | action | reward | done,
 *             R = 2 obs_dim + 3 goal_dim + act_dim + 2 floats
 *   ep_end    int64 [horizon, num_envs]: absolute time of the last transition of the entry's episode; the caller fills it with
 *             -1 before the first add (-1 = that episode is still running, or the slot was never written)
 *   ep_first  int64 [horizon, num_envs]: absolute time of that episode's first transition, written when the episode closes
 *   ep_start  int64 [num_envs]: absolute time each env's running episode began; zero before the first add
 *   clock     int64 [2] = {t, sample_calls}, zero before the first add: the add call stores time t and then advances t, the
 *             sample call draws with sample_calls and then advances it - both on the device, behind the kernel that read
 *             them, so the replays of a captured graph advance the clock as eager calls do
 * Neither call allocates, synchronises, or reads device memory from the host; each is two kernel launches. */
#define XARM_HER_FUTURE 0   /* goal time uniform on [time, episode end]: SB3's 'future' with online sampling */
#define XARM_HER_FINAL 1    /* goal time = episode end */
#define XARM_HER_EPISODE 2  /* goal time uniform on the part of the episode that is still in the ring */
typedef struct xarm_her_layout {
    int32_t num_envs;
    int32_t horizon;        /* ring slots, >= 2; at least twice the longest episode for every closed entry to stay reachable */
    int32_t obs_dim;
    int32_t goal_dim;
    int32_t act_dim;
} xarm_her_layout;          /* 20 bytes */
/* R, the floats of one record; XARM_E_INVALID for a NULL or unusable layout (dims < 1, horizon < 2, num_envs < 0) */
int xarm_her_record_floats(const xarm_her_layout *layout);
/* store one transition per env at slot t mod horizon ([num_envs, dim] float32 rows, rew float32 [num_envs], done uint8
 * [num_envs]; for a finished env next_obs / next_ag are the TERMINAL ones) and close the episodes of the envs with done set:
 * O(episode length) writes for those envs only.  num_envs == 0 launches nothing.  XARM_E_INVALID: unusable layout, or a NULL
 * pointer with num_envs > 0. */
int xarm_her_add(const xarm_her_layout *layout, float *ring, int64_t *ep_end, int64_t *ep_first, int64_t *ep_start, int64_t *clock,
                 const float *obs, const float *next_obs, const float *ag, const float *next_ag, const float *dg, const float *act,
                 const float *rew, const uint8_t *done_u8, void *stream);
/* draw `batch` rows uniformly from the stored entries of closed episodes (ep_end >= 0) into the [batch, dim] outputs, by
 * rejection: Philox(seed; row, sample_calls, attempt) proposes one of the min(t, horizon) num_envs stored entries, at most 64
 * times.  Rows [0, n_her) are relabelled: out_goal = next_achieved_goal of the same env at out_goal_time, chosen by `strategy`
 * inside the row's episode; the other rows keep the stored desired_goal.  out_rew is the STORED reward in every row: the caller
 * recomputes rows [0, n_her) with xarm_compute_reward on out_next_ag / out_goal, which are contiguous there.
 * out_env / out_time / out_goal_time (int64 [batch]) name the entry and the goal's source; out_ok_u8[b] = 0 marks a row whose 64
 * proposals all failed: its outputs are all zero and *fail_count_i64 (device, never cleared by this call) is incremented.
 * An empty buffer fails every row.  batch == 0 or num_envs == 0 launches nothing.  XARM_E_INVALID: unusable layout, batch < 0,
 * n_her outside [0, batch], unknown strategy, or a NULL pointer with batch > 0. */
int xarm_her_sample(const xarm_her_layout *layout, const float *ring, const int64_t *ep_end, const int64_t *ep_first, int64_t *clock,
                    uint64_t seed, int32_t strategy, int32_t batch, int32_t n_her, float *out_obs, float *out_next_obs, float *out_ag,
                    float *out_next_ag, float *out_goal, float *out_act, float *out_rew, uint8_t *out_done_u8, int64_t *out_env_i64,
                    int64_t *out_time_i64, int64_t *out_goal_time_i64, uint8_t *out_ok_u8, int64_t *fail_count_i64, void *stream);

/* ---- device-resident uniform replay (gym_xarm_amd/csrc/xarm_replay_core.h, xarm_k_replay.hip): SB3's plain
 * `ReplayBuffer` - every stored transition is sampled with the same probability, nothing is relabelled, running episodes
 * included - for the off-policy learners on a flat-observation env or on a goal env with a dense reward.  Like the HER calls
 * these need no env handle: the buffer is caller-owned DEVICE memory described by an xarm_replay_layout, the launches go to
 * `stream` on the caller's current device, and the messages of XARM_E_INVALID go to xarm_last_error(NULL).
 *   ring      float32 [horizon, num_envs, R], one record per (slot, env): obs | next_obs | action | reward | done | timeout,
 *             R = 2 D + act_dim + 3 floats.  D = obs_dim + 2 goal_dim is the learner's flat observation: the row
 *             observation | achieved_goal | desired_goal (goal_dim 0: the observation alone), and next_obs is
 *             next_observation | next_achieved_goal | desired_goal
 *   clock     int64 [2] = {t, sample_calls}, zero before the first add, advanced on the device as the HER clock is
 * Neither call allocates, synchronises, uses atomics or reads device memory from the host; each is two kernel launches. */
typedef struct xarm_replay_layout {
    int32_t num_envs;
    int32_t horizon;        /* ring slots per env, >= 1 */
    int32_t obs_dim;
    int32_t goal_dim;       /* 0: a flat-observation env, achieved / desired goal are not read */
    int32_t act_dim;
} xarm_replay_layout;       /* 20 bytes */
/* R, the floats of one record; XARM_E_INVALID for a NULL or unusable layout (obs_dim or act_dim < 1, goal_dim < 0, horizon < 1,
 * num_envs < 0) */
int xarm_replay_record_floats(const xarm_replay_layout *layout);
/* store one transition per env at slot t mod horizon ([num_envs, dim] float32 rows, rew float32 [num_envs], done uint8
 * [num_envs]; for a finished env next_obs / next_ag are the TERMINAL ones).  timeout_u8 (may be NULL = none) marks the envs whose
 * done is a time-limit truncation.  O(num_envs); num_envs == 0 launches nothing.  XARM_E_INVALID: unusable layout, or with
 * num_envs > 0 a NULL pointer other than timeout_u8 (ag / dg / next_ag may be NULL when goal_dim == 0). */
int xarm_replay_add(const xarm_replay_layout *layout, float *ring, int64_t *clock, const float *obs, const float *ag, const float *dg,
                    const float *next_obs, const float *next_ag, const float *act, const float *rew, const uint8_t *done_u8,
                    const uint8_t *timeout_u8 /* may be NULL */, void *stream);
/* draw `batch` rows uniformly from the min(t, horizon) num_envs stored transitions: row b takes entry
 * mulhi64(Philox(seed; b, sample_calls, 0, tag + sample_calls >> 32), min(t, horizon) num_envs) - one draw, no rejection.
 * The row is written as the learners take it: out_obs / out_next_obs [batch, D] - with stats (the normaliser's double
 * [2 D + 4], xarm_norm_obs's layout) column j is clamp((x - mean_j) / sqrt(var_j + eps), +-clip_obs) in float64, rounded to
 * float32 once, what xarm_norm_obs writes; with stats NULL the columns are copied - out_act [batch, act_dim], out_rew [batch] the
 * stored reward, out_done [batch] float32 = done && !(handle_timeout && timeout), out_use [batch] float32 = 1, or 0 with an
 * all-zero row while the buffer is empty.  out_env_i64 / out_time_i64 (int64 [batch], may be NULL) name the entry.
 * batch == 0 or num_envs == 0 launches nothing.  XARM_E_INVALID: unusable layout, batch < 0, with stats a clip_obs <= 0 or an
 * eps that is not finite and > 0, or with batch > 0 a NULL pointer other than stats / out_env_i64 / out_time_i64. */
int xarm_replay_sample(const xarm_replay_layout *layout, const float *ring, int64_t *clock, uint64_t seed, int32_t batch,
                       int32_t handle_timeout, const double *stats /* may be NULL */, double clip_obs, double eps, float *out_obs,
                       float *out_next_obs, float *out_act, float *out_rew, float *out_done, float *out_use,
                       int64_t *out_env_i64 /* may be NULL */, int64_t *out_time_i64 /* may be NULL */, void *stream);

/* ---- device-resident policy evaluation (gym_xarm_amd/csrc/xarm_eval_core.h, xarm_k_eval.hip): the episode
 * accounting of SB3's `evaluate_policy` for a batch of envs and the summary of its records.  Like the replay calls these need no
 * env handle: the state is caller-owned DEVICE memory described by an xarm_eval_layout, the launches go to `stream` on the
 * caller's current device, and the messages of XARM_E_INVALID go to xarm_last_error(NULL).
 * With E = num_envs, N = n_eval_episodes, q, r = divmod(N, E): env i contributes its first target[i] = (N + i) / E =
 * q + (i >= E - r) episodes after xarm_eval_begin (SB3's split), and episode k of env i is recorded at the fixed slot
 * base[i] + k, base[i] = q i + max(0, i - (E - r)) - env-major, whatever the order in which the envs finish.
 *   cur_ret   double [num_envs], cur_len int32 [num_envs]: return and length of the running episode
 *   count     int32 [num_envs]: records written per env
 *   remaining int32 [1]: N - records written; the only word a driver has to read back, and not on every step
 *   records   double [N, 3]: return (float64 sum of the float32 rewards), length, success
 * No call allocates, synchronises, uses floating-point atomics or reads device memory from the host; each is one launch and
 * can be captured in a graph.  XARM_E_INVALID: a NULL layout, num_envs < 0, n_eval_episodes < 1, or with num_envs > 0 a NULL
 * pointer other than keep_u8.  num_envs == 0 launches nothing. */
typedef struct xarm_eval_layout {
    int32_t num_envs;
    int32_t n_eval_episodes;    /* >= 1 */
} xarm_eval_layout;         /* 8 bytes */
/* zero cur_ret, cur_len, count and records; remaining = N */
int xarm_eval_begin(const xarm_eval_layout *layout, double *cur_ret, int32_t *cur_len_i32, int32_t *count_i32, int32_t *remaining_i32,
                    double *records, void *stream);
/* one env step: cur_ret += c rew, cur_len += c with c = keep_u8[i] != 0 (NULL: 1; lazy auto-reset hands ~resetting).  Where
 * done_u8[i] != 0: if count[i] < target[i] the record (cur_ret, cur_len, success_u8[i] != 0) is written and count[i] += 1; cur_ret
 * and cur_len are zeroed either way.  remaining falls by the records written in the call. */
int xarm_eval_step(const xarm_eval_layout *layout, double *cur_ret, int32_t *cur_len_i32, int32_t *count_i32, int32_t *remaining_i32,
                   double *records, const float *rew, const uint8_t *done_u8, const uint8_t *success_u8,
                   const uint8_t *keep_u8 /* may be NULL */, void *stream);
/* out (double [8]) = mean_reward, std_reward, mean_length, std_length, success_rate, min_reward, max_reward, n over the n records
 * written so far (a slot counts when its index inside its env is below count, not by its value); two-pass, population std as
 * np.std, in one fixed order: the same records give the same bits.  n == 0 gives NaN in every slot but the last. */
int xarm_eval_summary(const xarm_eval_layout *layout, const int32_t *count_i32, const double *records, double *out_f64, void *stream);

/* ---- device-resident VecNormalize + episode monitor (gym_xarm_amd/csrc/xarm_norm_core.h, xarm_k_norm.hip):
 * the running observation / return statistics, the normalised observation and reward and the Monitor's per-env return and length
 * of gym_xarm_amd/train.py (VecNormalize.step + EpisodeMonitor.update) in one stream-ordered call.  Like the HER calls these
 * need no env handle: the state is caller-owned DEVICE memory described by an xarm_norm_layout, the launches go to `stream` on
 * the caller's current device, and the messages of XARM_E_INVALID go to xarm_last_error(NULL).  D = obs_dim + 2 goal_dim.
 *   stats    double [2 D + 4]: obs_mean[D] | obs_var[D] | ret_mean | ret_var | obs_count | ret_count; before the first call the
 *            caller sets means 0, variances 1, counts 1e-4.  Every intermediate of the moments and of the normalisation is
 *            float64; the outputs are rounded to float32 once, after the clamp
 *   ret      float [num_envs]: running discounted return (zero at the start)
 *   ep_ret   float [num_envs], ep_len float [num_envs]: return and length of the running episode (zero at the start)
 *   ring     float [monitor_capacity, 3]: one (r, l, t) row per finished episode, episode k of the run at row k mod capacity
 *   n        int64 [1]: episodes recorded so far (zero at the start); the call advances it on the device
 *   work     xarm_norm_work_bytes() bytes, 8-byte aligned, scratch: every call rewrites what it reads, nothing survives a call
 * The result is a function of the inputs alone: rows are reduced in chunks of 128 in a fixed order, the chunks merged in index
 * order, no float atomics.  No call allocates, synchronises or reads device memory from the host; a call is three kernel
 * launches (the observation-only call with update == 0: one), num_envs == 0 launches nothing. */
#define XARM_NORM_MAX_DIM 96       /* D <= this: a chunk of 128 rows is staged in LDS */
typedef struct xarm_norm_layout {
    int32_t num_envs;
    int32_t obs_dim;
    int32_t goal_dim;           /* 0: `obs` is the whole row (a flat-observation env), achieved / desired goal are not read */
    int32_t monitor_capacity;   /* ring rows, >= num_envs: every env can finish in one call and no two rows may share a slot */
} xarm_norm_layout;             /* 16 bytes */
typedef struct xarm_norm_params {
    double clip_obs;            /* > 0 */
    double clip_reward;         /* > 0 */
    double eps;                 /* finite, > 0 */
    float gamma;                /* in [0, 1]; ret = ret * gamma + rew is a float32 multiply, then a float32 add */
    float t_seconds;            /* the t column of the rows this call appends.  Passed BY VALUE: the replays of a captured graph
                                 * repeat the value of the capture */
    int32_t update;             /* 0: the statistics are read, not updated (VecNormalize.training = False) */
} xarm_norm_params;             /* 40 bytes */
/* *bytes = size of `work` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (num_envs < 0, obs_dim < 1,
 * goal_dim < 0, D > XARM_NORM_MAX_DIM, monitor_capacity < max(1, num_envs)) */
int xarm_norm_work_bytes(const xarm_norm_layout *layout, int64_t *bytes);
/* the reset path, VecNormalize.reset: if params->update, merge the per-column moments of all num_envs rows into the observation
 * statistics; out_nobs[num_envs, D] = clamp((row - mean) / sqrt(var + eps), +-clip_obs) with the updated statistics, the row
 * being obs | achieved_goal | desired_goal ([num_envs, dim] float32 each; the kernels concatenate).  zero_ret != 0 also zeroes
 * ret.  Return statistics, monitor and n are not touched.  XARM_E_INVALID: unusable layout or params (eps not finite or <= 0,
 * a clip <= 0, gamma outside [0, 1]), or with num_envs > 0 a NULL stats / work / obs / out_nobs, a NULL achieved_goal /
 * desired_goal with goal_dim > 0, a NULL ret with zero_ret. */
int xarm_norm_obs(const xarm_norm_layout *layout, const xarm_norm_params *params, double *stats, float *ret, void *work,
                  const float *obs, const float *achieved_goal, const float *desired_goal, int32_t zero_ret, float *out_nobs,
                  void *stream);
/* one env step's bookkeeping, in VecNormalize.step + EpisodeMonitor.update order: ret = ret * gamma + rew; the moments of the
 * kept envs' ret merged into (ret_mean, ret_var, ret_count); out_nrew = clamp(rew / sqrt(ret_var + eps), +-clip_reward); ret = 0
 * where done; the kept rows' moments merged into the observation statistics; out_nobs as in xarm_norm_obs; ep_ret += rew c,
 * ep_len += c with c = keep as 0 / 1; every env with done_u8 != 0 appends (ep_ret, ep_len, t_seconds) at row (n + rank) mod
 * monitor_capacity, rank = its position among this call's finished envs in env order, and its ep_ret / ep_len are zeroed;
 * n += finished envs.  keep_u8 (may be NULL = every env) marks the envs whose row feeds the statistics and the episode sums: under
 * lazy auto-reset, the envs that are not spending the call on a reset tick.  A call without kept rows leaves stats bit for bit
 * unchanged, as does update == 0.  XARM_E_INVALID: as xarm_norm_obs, or a NULL pointer other than keep_u8 with num_envs > 0. */
int xarm_norm_step(const xarm_norm_layout *layout, const xarm_norm_params *params, double *stats, float *ret, float *ep_ret,
                   float *ep_len, float *ring, int64_t *n_i64, void *work, const float *obs, const float *achieved_goal,
                   const float *desired_goal, const float *rew, const uint8_t *done_u8, const uint8_t *keep_u8 /* may be NULL */,
                   float *out_nobs, float *out_nrew, void *stream);

/* ---- device-resident MlpPolicy (gym_xarm_amd/csrc/xarm_policy_core.h, xarm_k_policy.hip): the forward of
 * gym_xarm_amd/train.py's ActorCritic - two 64-64 tanh towers and a state-independent log_std - with the Gaussian sample, the
 * clamp to [-1, 1], the log-probability and the value, in ONE kernel launch per call (a stochastic call is followed by a
 * one-thread launch that advances `calls`).  Like the normaliser calls it needs no env handle; everything is caller-owned DEVICE
 * memory, the launches go to `stream` on the caller's current device, and the messages of XARM_E_INVALID go to
 * xarm_last_error(NULL).  D = obs_dim + 2 goal_dim.
 *   weights  the 13 float32 parameter tensors, W in [out, in] row-major layout (torch.nn.Linear): W1 [64, D], b1 [64], W2 [64, 64],
 *            b2 [64], W3 [act_dim, 64] (value tower: [1, 64]), b3, and log_std [act_dim].  They are read in place on every call;
 *            b1, W2, b2 and W3 must be 16-byte aligned (they are read in 16-byte pieces).
 *   stats    NULL, or the normaliser's double [2 D + 4]: the row is then normalised inline with these FROZEN statistics -
 *            clamp((x - mean) / sqrt(var + eps), +-clip_obs) in float64, rounded to float32 once - and never updated
 *   calls    int64 [1], zero at the start: the noise of a stochastic call is keyed by (seed, row_offset + row, *calls, column
 *            block); the call advances it on the device behind the kernel that read it, so the replays of a captured graph draw
 *            fresh noise.  A deterministic call neither reads nor advances it.
 *   outputs  out_action [num_envs, act_dim] = mean + exp(log_std) z (mean when deterministic), out_env_action = out_action clamped
 *            to [-1, 1], out_logp [num_envs] (may be NULL) = sum over columns of -z^2 / 2 - log_std - log(2 pi) / 2, out_value
 *            [num_envs] (may be NULL: the value tower is then skipped)
 * Every dot product is a float32 fused-multiply-add chain from the bias in a fixed order, the elementary functions are spelled
 * out in float32 operations: a row's result depends on that row, the weights, seed, row_offset + row and *calls alone - not on the
 * batch it is in.  No call allocates, synchronises or reads device memory from the host; num_envs == 0 launches nothing. */
#define XARM_POLICY_MAX_DIM 96     /* D <= this */
#define XARM_POLICY_MAX_ACT 16     /* 1 <= act_dim <= this */
#define XARM_POLICY_HIDDEN 64      /* the only hidden width */
typedef struct xarm_policy_layout {
    int32_t num_envs;
    int32_t obs_dim;
    int32_t goal_dim;           /* 0: `obs` is the whole row, achieved / desired goal are not read */
    int32_t act_dim;
    int32_t hidden;             /* XARM_POLICY_HIDDEN */
    int64_t row_offset;         /* global index of row 0 (>= 0): a shard of a larger batch draws the noise of its global rows */
} xarm_policy_layout;           /* 32 bytes (4 bytes of padding before row_offset) */
typedef struct xarm_policy_params {
    uint64_t seed;
    double clip_obs;            /* > 0; read with stats only */
    double eps;                 /* finite, > 0; read with stats only */
    int32_t deterministic;      /* != 0: action = mean, no noise is drawn, calls is not advanced */
} xarm_policy_params;           /* 32 bytes */
typedef struct xarm_policy_weights {
    const float *pi_w1, *pi_b1, *pi_w2, *pi_b2, *pi_w3, *pi_b3;
    const float *vf_w1, *vf_b1, *vf_w2, *vf_b2, *vf_w3, *vf_b3;   /* read only when out_value is set */
    const float *log_std;
} xarm_policy_weights;          /* 13 device pointers */
/* XARM_E_INVALID: NULL layout / params / weights, num_envs < 0, obs_dim < 1, goal_dim < 0, D > XARM_POLICY_MAX_DIM, act_dim outside
 * [1, XARM_POLICY_MAX_ACT], hidden != XARM_POLICY_HIDDEN, row_offset < 0, with stats an eps that is not finite and > 0 or a
 * clip_obs <= 0, or with num_envs > 0 a NULL policy weight, log_std, obs, out_action or out_env_action, a NULL achieved_goal /
 * desired_goal with goal_dim > 0, a NULL value weight with out_value set, a misaligned b1 / W2 / b2 / W3, a NULL calls with
 * deterministic == 0. */
int xarm_policy_act(const xarm_policy_layout *layout, const xarm_policy_params *params, const xarm_policy_weights *weights,
                    const double *stats /* may be NULL */, int64_t *calls_i64, const float *obs, const float *achieved_goal,
                    const float *desired_goal, float *out_action, float *out_env_action, float *out_logp /* may be NULL */,
                    float *out_value /* may be NULL */, void *stream);

/* ---- device-resident A2C update (gym_xarm_amd/csrc/xarm_a2c_core.h, xarm_k_a2c.hip): one update of
 * gym_xarm_amd/train.py's loop - bootstrap value, n-step returns, the backward of both towers, torch's clip_grad_norm_ and
 * torch's RMSprop (no momentum, not centred, no weight decay) - as six stream-ordered launches on `stream`, with no allocation,
 * no host read and no side stream.  Everything is caller-owned float32 DEVICE memory, row-major; T = n_steps, E = num_envs,
 * D = obs_dim, A = act_dim.
 *   obs [T, E, D] (already normalised, flat), action [T, E, A], reward [T, E], done [T, E] (non-zero cuts the return),
 *   use [T, E] (may be NULL = all ones), last_obs [E, D]
 *   ret_T = value(last_obs); ret_k = fmaf(gamma (1 - done_k), ret_k+1, reward_k) in float32; adv = ret - value(obs) (no gradient
 *   through ret or adv); n_use = max(sum use, 1);
 *   loss = -sum(adv logp use) / n_use + vf_coef sum((ret - value)^2 use) / n_use - ent_coef sum_c(log_std_c + 1/2 + log(2 pi) / 2)
 *   norm = sqrt(sum g^2) over the 13 tensors, g *= min(1, max_grad_norm / (norm + 1e-6));
 *   sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps)
 *   weights     the policy's 13 tensors (xarm_policy_weights; the same alignment rule), READ AND WRITTEN in place
 *   square_avg  RMSprop's 13 state tensors in the same shapes, read and written in place
 *   workspace   xarm_a2c_workspace_bytes() bytes, 16-byte aligned; holds nothing between calls
 *   out_returns [T, E], out_grad [P] (the gradient before the clip, after the 1 / n_use factor, the 13 tensors one after the other
 *               in the struct's order), out_stats [8] = policy_loss, value_loss, entropy, grad_norm, n_use, 0, 0, 0: each may be NULL
 * Sums over rows run in a fixed order through per-workgroup partials (no floating-point atomics): the same inputs give the same
 * bits.  num_envs == 0 launches nothing. */
typedef struct xarm_a2c_layout {
    int32_t num_envs;
    int32_t n_steps;            /* >= 1; n_steps * num_envs < 2^31 */
    int32_t obs_dim;            /* D, 1 .. XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_POLICY_MAX_ACT */
    int32_t hidden;             /* XARM_POLICY_HIDDEN */
} xarm_a2c_layout;              /* 20 bytes */
typedef struct xarm_a2c_params {
    double gamma;               /* [0, 1] */
    double lr;                  /* >= 0 */
    double alpha;               /* [0, 1) */
    double eps;                 /* > 0 */
    double vf_coef;
    double ent_coef;
    double max_grad_norm;       /* > 0 */
} xarm_a2c_params;              /* 56 bytes */
/* *bytes = size of `workspace` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_a2c_workspace_bytes(const xarm_a2c_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: NULL layout / params / weights / square_avg, num_envs < 0, n_steps < 1, n_steps * num_envs >= 2^31, obs_dim outside
 * [1, XARM_POLICY_MAX_DIM], act_dim outside [1, XARM_POLICY_MAX_ACT], hidden != XARM_POLICY_HIDDEN, gamma outside [0, 1], lr < 0,
 * alpha outside [0, 1), eps <= 0, max_grad_norm <= 0, a vf_coef or ent_coef that is not finite, or with num_envs > 0 a NULL weight or
 * square_avg tensor, a misaligned b1 / W2 / b2 / W3 of `weights`, a NULL obs / action / reward / done / last_obs, a NULL or not
 * 16-byte aligned workspace. */
int xarm_a2c_update(const xarm_a2c_layout *layout, const xarm_a2c_params *params, const xarm_policy_weights *weights,
                    const xarm_policy_weights *square_avg, const float *obs, const float *action, const float *reward,
                    const float *done, const float *use /* may be NULL */, const float *last_obs, void *workspace,
                    float *out_returns /* may be NULL */, float *out_grad /* may be NULL */, float *out_stats /* may be NULL */,
                    void *stream);

/* ---- device-resident PPO update (gym_xarm_amd/csrc/xarm_ppo_core.h, xarm_k_ppo.hip): one PPO.train() of
 * stable-baselines3 on a stored rollout - GAE(lambda), n_epochs passes over shuffled minibatches, per-minibatch advantage
 * normalisation, the clipped surrogate, the backward of both towers, torch's clip_grad_norm_ and torch's Adam (no amsgrad, no weight
 * decay) - as 4 + 3 S stream-ordered launches on `stream`, S = n_epochs * ceil(N / batch_size), N = n_steps * num_envs, with no
 * allocation, no host read and no side stream.  Memory, shapes and the A2C arguments are those of xarm_a2c_update.
 *   v_k = value(obs_k), v_T = value(last_obs) and old_logp (the log-probability of the stored action) under the weights at call start;
 *   keep = 1 - [done_k != 0]; delta = fmaf(gamma keep, v_k+1, reward_k) - v_k; adv_k = fmaf(gamma lambda keep, adv_k+1, delta), adv_T = 0;
 *   ret_k = adv_k + v_k (no gradient through adv or ret)
 *   step s = epoch * M + m reads the rows perm[epoch][m * B .. min((m + 1) * B, N)); an entry outside [0, N) counts as a row with
 *   use = 0 and nothing is read through it.  n = sum use over the step's rows, n_use = max(n, 1);
 *   A^ = (adv - mu) / (sigma + 1e-8) with the step's float64 mean and unbiased standard deviation over its used rows (adv itself when
 *   n <= 1 or normalize_advantage == 0); rho = exp(logp - old_logp);
 *   loss = -sum(min(rho A^, clamp(rho, 1 - clip_range, 1 + clip_range) A^) use) / n_use + vf_coef sum((ret - value)^2 use) / n_use
 *          - ent_coef sum_c(log_std_c + 1/2 + log(2 pi) / 2), logp and value under the weights of the step;
 *   the clip of A2C; t = ++step; m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   exp_avg, exp_avg_sq  Adam's 13 + 13 state tensors in the weights' shapes, read and written in place
 *   step_i64    device int64 [1]: Adam's step count, advanced on the device by the number of APPLIED steps (a replayed graph continues
 *               the count): S, or fewer when target_kl stops the call (below)
 *   old_logp    [T, E], may be NULL (computed at call start); perm int32 [n_epochs, N], each row a permutation of 0 .. N - 1
 *   workspace   xarm_ppo_workspace_bytes() bytes, 16-byte aligned; holds nothing between calls
 *   out_adv / out_returns [T, E], out_grad [P] (step 0's gradient before the clip), out_stats [S, 8], row s = policy_loss, value_loss,
 *               entropy, grad_norm, n_use, approx_kl = sum(((rho - 1) - log rho) use) / n_use, clip_fraction =
 *               sum([|rho - 1| > clip_range] use) / n_use, stopped (0: the step was applied, 1: it was not): each may be NULL
 * The two options of xarm_ppo_update_opt (both 0, or options == NULL: the update above, bit for bit):
 *   clip_range_vf = c > 0   with v0 the row's value at call start and v its value under the step's weights: inside = |v - v0| <= c;
 *               vp = inside ? v : (v > v0 ? v0 + c : v0 - c); the value loss sums (ret - vp)^2 use, and the value's output delta is
 *               2 vf_coef ((v - ret) use) inside and 0 outside (stable-baselines3's clip_range_vf: torch.clamp's backward is inclusive)
 *   target_kl > 0   after step s's sums over rows, with kl_s the float32 that goes into out_stats[s, 5]: the step trips when
 *               (double)kl_s > 1.5 target_kl.  A step that trips and every later step of the call is not applied: step_i64 is not
 *               advanced and no parameter or Adam state is written (stable-baselines3's break before the optimiser step).  The
 *               tripping row of out_stats keeps its sums, with grad_norm = 0 and stopped = 1; later rows are 0 but for stopped = 1.
 *               The decision is a flag in the workspace that a launch at call start clears and every launch of a step reads: still
 *               no host read, and a captured graph replays it.  out_grad is step 0's gradient also when step 0 trips.
 * No floating-point atomics: the same inputs and perm give the same bits.  num_envs == 0 launches nothing. */
typedef struct xarm_ppo_layout {
    int32_t num_envs;
    int32_t n_steps;            /* >= 1; n_steps * num_envs < 2^31 */
    int32_t obs_dim;            /* D, 1 .. XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_POLICY_MAX_ACT */
    int32_t hidden;             /* XARM_POLICY_HIDDEN */
    int32_t n_epochs;           /* >= 1 */
    int32_t batch_size;         /* >= 1; n_epochs * ceil(N / batch_size) <= 4096 */
} xarm_ppo_layout;              /* 28 bytes */
typedef struct xarm_ppo_params {
    double gamma;               /* [0, 1] */
    double gae_lambda;          /* [0, 1] */
    double clip_range;          /* > 0 */
    double lr;                  /* >= 0 */
    double beta1;               /* [0, 1) */
    double beta2;               /* [0, 1) */
    double eps;                 /* > 0 */
    double vf_coef;
    double ent_coef;
    double max_grad_norm;       /* > 0 */
    int32_t normalize_advantage;
} xarm_ppo_params;              /* 88 bytes */
typedef struct xarm_ppo_options {
    double clip_range_vf;       /* 0 = off; otherwise finite and > 0 */
    double target_kl;           /* 0 = off; otherwise finite and > 0 */
} xarm_ppo_options;             /* 16 bytes */
/* *bytes = size of `workspace` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_ppo_workspace_bytes(const xarm_ppo_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: everything xarm_a2c_update refuses (with exp_avg / exp_avg_sq in square_avg's place), n_epochs < 1, batch_size < 1,
 * n_epochs * ceil(N / batch_size) > 4096, gae_lambda outside [0, 1], a clip_range that is not finite or <= 0, beta1 or beta2 outside
 * [0, 1), or with num_envs > 0 a NULL exp_avg / exp_avg_sq tensor, a NULL step_i64, a NULL perm. */
int xarm_ppo_update(const xarm_ppo_layout *layout, const xarm_ppo_params *params, const xarm_policy_weights *weights,
                    const xarm_policy_weights *exp_avg, const xarm_policy_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *action, const float *reward, const float *done, const float *use /* may be NULL */,
                    const float *last_obs, const float *old_logp /* may be NULL */, const int32_t *perm, void *workspace,
                    float *out_adv /* may be NULL */, float *out_returns /* may be NULL */, float *out_grad /* may be NULL */,
                    float *out_stats /* may be NULL */, void *stream);
/* xarm_ppo_update (which is this call with options == NULL) with the options above.  XARM_E_INVALID besides: an option that is negative,
 * NaN or infinite. */
int xarm_ppo_update_opt(const xarm_ppo_layout *layout, const xarm_ppo_params *params, const xarm_policy_weights *weights,
                        const xarm_policy_weights *exp_avg, const xarm_policy_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                        const float *action, const float *reward, const float *done, const float *use /* may be NULL */,
                        const float *last_obs, const float *old_logp /* may be NULL */, const int32_t *perm, void *workspace,
                        float *out_adv /* may be NULL */, float *out_returns /* may be NULL */, float *out_grad /* may be NULL */,
                        float *out_stats /* may be NULL */, const xarm_ppo_options *options /* NULL = none */, void *stream);

/* ---- device-resident SAC update (gym_xarm_amd/csrc/xarm_sac_core.h, xarm_k_sac.hip): ONE gradient step of
 * stable-baselines3's SAC.train() on a batch drawn from a replay buffer - the squashed-Gaussian actor on obs and next_obs, the
 * entropy coefficient's step, the soft target, the step of both critics, the actor's step through the updated critics and the
 * Polyak step of the targets - as six stream-ordered launches on `stream`, with no allocation, no host read, no atomics and no side
 * stream.  Everything is caller-owned float32 DEVICE memory, row-major; B = batch_size, D = obs_dim, A = act_dim.
 *   model    actor D -> 64 -> 64 -> 2A (tanh; outputs 0 .. A-1 the mean, A .. 2A-1 log_std), q1 / q2 / q1_target / q2_target
 *            D + A -> 64 -> 64 -> 1 (tanh) on the row obs | action, log_alpha [1]; W in [out, in] layout as xarm_policy_weights
 *   actor    ls = clamp(log_std, -20, 2); u = mean + exp(ls) z; a = tanh(u);
 *            logp = sum_c(-z_c^2 / 2 - ls_c - log(2 pi) / 2) - sum_c log(1 - a_c^2 + 1e-6)
 *   step     alpha = auto_ent_coef ? exp(log_alpha) : ent_coef, read before anything is stepped; use NULL = all ones;
 *            n_use = max(sum use, 1); every mean below is sum(. use) / n_use
 *            a_pi, logp_pi = actor(obs; z_pi);   a', logp' = actor(next_obs; z_next)
 *            alpha_loss = -mean(log_alpha (logp_pi + target_entropy)), Adam on log_alpha (auto_ent_coef only)
 *            y = reward + gamma (1 - done) (min(q1_target, q2_target)(next_obs | a') - alpha logp')      (no gradient)
 *            critic_loss = (mean((q1(obs | action) - y)^2) + mean((q2(obs | action) - y)^2)) / 2, Adam on q1 and q2
 *            actor_loss = mean(alpha logp_pi - min(q1, q2)(obs | a_pi)) under the stepped critics, Adam on the actor
 *            target = (1 - tau) target + tau critic
 *            Adam: t = ++step; m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g^2;
 *            p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps); no gradient clip
 *   weights  the 31 tensors, READ AND WRITTEN in place (b1, W2, b2 and W3 of each tower 16-byte aligned)
 *   exp_avg, exp_avg_sq  Adam's state of actor, q1, q2 and log_alpha in the same struct; the target fields are not read
 *   step_i64 device int64 [1]: Adam's step count of the three optimisers, advanced by one on the device per call
 *   noise_pi / noise_next [B, A]: the step's z.  NULL: Philox keyed by (seed, row, *step_i64 at call start, a tag per stream of noise)
 *   workspace   xarm_sac_workspace_bytes() bytes, 16-byte aligned; holds nothing between calls
 *   out_grad [P] (actor's 6 tensors, q1's, q2's, log_alpha: the gradients after the 1 / n_use factor), out_dqda [2, B, A] (d q_i /
 *   d action at obs | a_pi under the stepped critics), out_target [B] (y), out_stats [8] = critic_loss, actor_loss, alpha_loss, alpha,
 *   mean logp_pi, mean min-Q(obs | a_pi), n_use, 0: each may be NULL
 * xarm_sac_act is the rollout / deployment call: out_action [B, A] = tanh(u) (tanh(mean) when deterministic), out_logp [B] (may be
 * NULL), noise as xarm_policy_act draws it - Philox keyed by (seed, row_offset + row, *calls, column block) - and a stochastic call
 * is followed by a one-thread launch that advances `calls`.  A row's result does not depend on the batch it is in.
 * Sums over rows run in a fixed order through per-workgroup partials: the same inputs give the same bits.  batch_size == 0
 * launches nothing. */
#define XARM_SAC_MAX_ACT 8         /* 1 <= act_dim <= this: the actor's 2 act_dim outputs fill XARM_POLICY_MAX_ACT columns */
typedef struct xarm_sac_layout {
    int32_t batch_size;         /* B >= 0: rows of the call */
    int32_t obs_dim;            /* D >= 1, D + act_dim <= XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_SAC_MAX_ACT */
    int32_t hidden;             /* XARM_POLICY_HIDDEN */
    int64_t row_offset;         /* xarm_sac_act: global index of row 0 (>= 0) */
} xarm_sac_layout;              /* 24 bytes */
typedef struct xarm_sac_params {
    uint64_t seed;
    double gamma;               /* [0, 1] */
    double lr;                  /* >= 0 */
    double tau;                 /* [0, 1] */
    double ent_coef;            /* the fixed alpha (finite, >= 0); read when auto_ent_coef == 0 */
    double target_entropy;      /* finite; stable-baselines3's default is -act_dim */
    double beta1;               /* [0, 1) */
    double beta2;               /* [0, 1) */
    double eps;                 /* > 0 */
    int32_t auto_ent_coef;      /* != 0: alpha = exp(log_alpha) and log_alpha is trained */
    int32_t deterministic;      /* xarm_sac_act: != 0: action = tanh(mean), no noise is drawn, calls is not advanced */
} xarm_sac_params;              /* 80 bytes */
typedef struct xarm_sac_weights {
    const float *actor[6];      /* W1 [64, D], b1 [64], W2 [64, 64], b2 [64], W3 [2 A, 64], b3 [2 A] */
    const float *q1[6];         /* W1 [64, D + A], b1, W2, b2, W3 [1, 64], b3 [1] */
    const float *q2[6];
    const float *q1_target[6];
    const float *q2_target[6];
    const float *log_alpha;     /* [1] */
} xarm_sac_weights;             /* 31 device pointers */
/* *bytes = size of `workspace` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_sac_workspace_bytes(const xarm_sac_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: NULL layout / params / weights, batch_size < 0, obs_dim < 1, act_dim outside [1, XARM_SAC_MAX_ACT],
 * obs_dim + act_dim > XARM_POLICY_MAX_DIM, hidden != XARM_POLICY_HIDDEN, row_offset < 0, or with batch_size > 0 a NULL or misaligned
 * actor tensor, a NULL obs or out_action, a NULL calls with deterministic == 0. */
int xarm_sac_act(const xarm_sac_layout *layout, const xarm_sac_params *params, const xarm_sac_weights *weights, int64_t *calls_i64,
                 const float *obs, float *out_action, float *out_logp /* may be NULL */, void *stream);
/* XARM_E_INVALID: everything the layout check of xarm_sac_act refuses, NULL exp_avg / exp_avg_sq, gamma or tau outside [0, 1], lr < 0,
 * an ent_coef that is not finite and >= 0, a target_entropy that is not finite, beta1 or beta2 outside [0, 1), eps <= 0, or with
 * batch_size > 0 a NULL weight tensor, a NULL exp_avg / exp_avg_sq tensor of actor, q1, q2 or log_alpha, a misaligned b1 / W2 / b2 /
 * W3, a NULL step_i64 / obs / next_obs / action / reward / done, a NULL or not 16-byte aligned workspace. */
int xarm_sac_update(const xarm_sac_layout *layout, const xarm_sac_params *params, const xarm_sac_weights *weights,
                    const xarm_sac_weights *exp_avg, const xarm_sac_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *next_obs, const float *action, const float *reward, const float *done,
                    const float *use /* may be NULL */, const float *noise_pi /* may be NULL */,
                    const float *noise_next /* may be NULL */, void *workspace, float *out_grad /* may be NULL */,
                    float *out_dqda /* may be NULL */, float *out_target /* may be NULL */, float *out_stats /* may be NULL */,
                    void *stream);

/* ---- wide device-resident SAC (gym_xarm_amd/csrc/xarm_sacw_core.h, xarm_k_sacw.hip): the step of xarm_sac_update and
 * the act call of xarm_sac_act for equal-width towers of n_hidden = 2 or 3 hidden layers of hidden = 64, 128, 192 or 256 units, tanh
 * or ReLU - stable-baselines3's `policy_kwargs=dict(net_arch=[256, 256, 256])` among them.  Arguments and semantics are xarm_sac_*'s
 * with these changes: the layout names hidden, n_hidden and activation; a tower is 2 (n_hidden + 1) pointers W1, b1, ..., W_out, b_out
 * (nn.Linear's [out, in] layout) in arrays sized for n_hidden = 3, the unused tail ignored; xarm_sacw_act takes a workspace too (the
 * activations of a layer-by-layer forward live there); xarm_sacw_update has one more optional output, out_q [2, B] = q1 and q2 at
 * obs | action as the critic stage computes them.  out_grad [P] holds the actor's 2 (n_hidden + 1) tensors, q1's, q2's, log_alpha.
 * The dense work is a chain of per-layer GEMM launches on v_mfma_f32_32x32x2_f32 - 6 n_hidden + 11 launches per step, n_hidden + 2 (+ the
 * tick) per act call, a function of n_hidden alone - with no allocation, no host read, no atomics and no side stream.  Sums over rows
 * run in a fixed order (float32 within one of at most 16 contiguous row ranges, float64 across them): the same inputs give the same
 * bits.  Out of scope: unequal widths, n_critics != 2, use_sde.  batch_size == 0 launches nothing. */
#define XARM_SACW_MAX_LAYERS 3    /* n_hidden is 2 or 3 */
#define XARM_SACW_MAX_HIDDEN 256  /* hidden is 64, 128, 192 or 256 */
#define XARM_SACW_TANH 0
#define XARM_SACW_RELU 1
typedef struct xarm_sacw_layout {
    int32_t batch_size;         /* B >= 0: rows of the call */
    int32_t obs_dim;            /* D >= 1, D + act_dim <= XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_SAC_MAX_ACT */
    int32_t hidden;             /* 64, 128, 192 or 256 */
    int32_t n_hidden;           /* 2 or 3 */
    int32_t activation;         /* XARM_SACW_TANH or XARM_SACW_RELU */
    int64_t row_offset;         /* xarm_sacw_act: global index of row 0 (>= 0) */
} xarm_sacw_layout;             /* 32 bytes */
typedef struct xarm_sacw_weights {
    const float *actor[2 * (XARM_SACW_MAX_LAYERS + 1)];     /* W1 [H, D], b1 [H], W2 [H, H], b2 [H], (W3 [H, H], b3 [H],) W_out [2 A, H], b_out [2 A] */
    const float *q1[2 * (XARM_SACW_MAX_LAYERS + 1)];        /* W1 [H, D + A], b1, ..., W_out [1, H], b_out [1] */
    const float *q2[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *q1_target[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *q2_target[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *log_alpha;     /* [1] */
} xarm_sacw_weights;            /* 41 device pointers */
/* *bytes = size of `workspace` for this layout (of either call).  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_sacw_workspace_bytes(const xarm_sacw_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: what xarm_sac_act refuses, with hidden outside {64, 128, 192, 256}, n_hidden outside {2, 3} or activation outside
 * {XARM_SACW_TANH, XARM_SACW_RELU} in place of hidden != 64; with batch_size > 0 a NULL actor tensor, a tensor from b1 to W_out that is
 * not 16-byte aligned, a NULL or not 16-byte aligned workspace. */
int xarm_sacw_act(const xarm_sacw_layout *layout, const xarm_sac_params *params, const xarm_sacw_weights *weights, int64_t *calls_i64,
                  const float *obs, void *workspace, float *out_action, float *out_logp /* may be NULL */, void *stream);
/* XARM_E_INVALID: what xarm_sac_update refuses, with the layout check above. */
int xarm_sacw_update(const xarm_sacw_layout *layout, const xarm_sac_params *params, const xarm_sacw_weights *weights,
                     const xarm_sacw_weights *exp_avg, const xarm_sacw_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                     const float *next_obs, const float *action, const float *reward, const float *done,
                     const float *use /* may be NULL */, const float *noise_pi /* may be NULL */,
                     const float *noise_next /* may be NULL */, void *workspace, float *out_grad /* may be NULL */,
                     float *out_dqda /* may be NULL */, float *out_target /* may be NULL */, float *out_stats /* may be NULL */,
                     float *out_q /* may be NULL */, void *stream);

/* ---- device-resident TD3 (gym_xarm_amd/csrc/xarm_td3_core.h, xarm_k_td3.hip): ONE gradient step of stable-baselines3's
 * TD3.train() on a batch drawn from a replay buffer, on xarm_sacw's per-layer f32 MFMA GEMM chain, for the shapes of xarm_sacw_layout
 * (equal widths of 64, 128, 192 or 256 units, two or three hidden layers, tanh or ReLU).  Everything is caller-owned float32 DEVICE
 * memory, row-major; B = batch_size, D = obs_dim, A = act_dim.
 *   model    actor and actor_target D -> H x L -> A with tanh on the output; q1 / q2 / q1_target / q2_target D + A -> H x L -> 1 on the
 *            row obs | action; a tower is 2 (n_hidden + 1) pointers W1, b1, ..., W_out, b_out as in xarm_sacw_weights
 *   step     t = *step_i64 at call start; use NULL = all ones; n_use = max(sum use, 1); every mean is sum(. use) / n_use
 *            a' = clamp(tanh(actor_target(next_obs)) + clamp(target_policy_noise z, -target_noise_clip, target_noise_clip), -1, 1)
 *            y = reward + gamma (1 - done) min(q1_target, q2_target)(next_obs | a')                          (no gradient)
 *            critic_loss = mean((q1(obs | action) - y)^2) + mean((q2(obs | action) - y)^2), Adam on q1 and q2 at count t + 1
 *            when (t + 1) % policy_delay == 0, decided on the device:
 *              actor_loss = -mean(q1(obs | tanh(actor(obs)))) under the stepped q1, Adam on the actor at count (t + 1) / policy_delay
 *              target = (1 - tau) target + tau net for actor_target, q1_target and q2_target (the stepped critics)
 *   weights  the six towers, READ AND WRITTEN in place (b1 .. W_out of each tower 16-byte aligned)
 *   exp_avg, exp_avg_sq  Adam's state of actor, q1 and q2 in the same struct; the target fields are not read
 *   step_i64 device int64 [1]: the calls so far (the critics' Adam count), advanced by one on the device per call
 *   noise_next [B, A]: the step's z.  NULL: Philox keyed by (seed, row_offset + row, t), the noise stream 1 of xarm_sacw_update
 *   workspace   xarm_td3_workspace_bytes() bytes, 16-byte aligned; holds nothing between calls
 *   out_grad [P] (actor's tensors, q1's, q2's: the gradients after the 1 / n_use factor; the actor's part is left as it is on a call
 *   without an actor step), out_target [B] (y), out_q [2, B] (q1, q2 at obs | action), out_dqda [B, A] (d q1 / d action at obs | a_pi
 *   under the stepped q1; written on a call with an actor step), out_stats [8] = critic_loss, actor_loss, mean q1(obs | a_pi), mean y,
 *   n_use, actor_stepped, 0, 0 - actor_loss and the mean q1 are left as they are on a call without an actor step, so a row that starts
 *   at zero repeats the last actor step's values: each may be NULL
 * A call is 7 n_hidden + 14 launches on `stream`, on delayed and undelayed calls alike (the actor phase's launches return after one
 * uniform read of a flag in the workspace), with no allocation, no host read, no atomics and no side stream: it can be captured and
 * replayed.  Sums run in xarm_sacw_update's fixed order: the same inputs give the same bits.
 * xarm_td3_act is the rollout / deployment call, by params->mode: 0 out_action [B, A] = tanh(actor(obs)); 1 clamp(tanh(actor(obs)) +
 * action_noise z, -1, 1) with z as xarm_sacw_act draws it - Philox keyed by (seed, row_offset + row, *calls, column block); 2 uniform
 * on [-1, 1) from Philox under the same key, obs and the weights not read.  Modes 1 and 2 are followed by a one-thread launch that
 * advances `calls`.  A row's result does not depend on the batch it is in.  n_hidden + 2 launches (1 in mode 2; + the tick).
 * Out of scope: DDPG and n_critics != 2, unequal widths, a fourth hidden layer, widths above 256, use_sde.  batch_size == 0 launches
 * nothing. */
typedef struct xarm_td3_params {
    uint64_t seed;
    double gamma;               /* [0, 1] */
    double lr;                  /* >= 0 */
    double tau;                 /* [0, 1] */
    double beta1;               /* [0, 1) */
    double beta2;               /* [0, 1) */
    double eps;                 /* > 0 */
    double target_policy_noise; /* finite, >= 0 */
    double target_noise_clip;   /* finite, >= 0 */
    double action_noise;        /* xarm_td3_act, mode 1: finite, >= 0 */
    int32_t policy_delay;       /* >= 1 */
    int32_t mode;               /* xarm_td3_act: 0 deterministic, 1 Gaussian, 2 uniform */
} xarm_td3_params;              /* 88 bytes */
typedef struct xarm_td3_weights {
    const float *actor[2 * (XARM_SACW_MAX_LAYERS + 1)];     /* W1 [H, D], b1 [H], W2 [H, H], b2 [H], (W3 [H, H], b3 [H],) W_out [A, H], b_out [A] */
    const float *q1[2 * (XARM_SACW_MAX_LAYERS + 1)];        /* W1 [H, D + A], b1, ..., W_out [1, H], b_out [1] */
    const float *q2[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *actor_target[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *q1_target[2 * (XARM_SACW_MAX_LAYERS + 1)];
    const float *q2_target[2 * (XARM_SACW_MAX_LAYERS + 1)];
} xarm_td3_weights;             /* 48 device pointers */
/* *bytes = size of `workspace` for this layout (of either call).  XARM_E_INVALID: NULL argument or unusable layout (xarm_sacw's). */
int xarm_td3_workspace_bytes(const xarm_sacw_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: what xarm_sacw_act's layout check refuses, NULL params / weights, a mode outside {0, 1, 2}, a policy_delay < 1, a
 * negative noise or clip, tau or gamma outside [0, 1]; with batch_size > 0 a NULL or misaligned actor tensor or a NULL obs (modes 0 and
 * 1), a NULL out_action, a NULL calls with mode != 0, a NULL or not 16-byte aligned workspace. */
int xarm_td3_act(const xarm_sacw_layout *layout, const xarm_td3_params *params, const xarm_td3_weights *weights, int64_t *calls_i64,
                 const float *obs, void *workspace, float *out_action, void *stream);
/* XARM_E_INVALID: every case xarm_sacw_update refuses (with the six towers of xarm_td3_weights in place of its five and log_alpha),
 * policy_delay < 1, a negative or non-finite target_policy_noise, target_noise_clip or action_noise, tau outside [0, 1].  All checks
 * come before any launch. */
int xarm_td3_update(const xarm_sacw_layout *layout, const xarm_td3_params *params, const xarm_td3_weights *weights,
                    const xarm_td3_weights *exp_avg, const xarm_td3_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                    const float *next_obs, const float *action, const float *reward, const float *done,
                    const float *use /* may be NULL */, const float *noise_next /* may be NULL */, void *workspace,
                    float *out_grad /* may be NULL */, float *out_target /* may be NULL */, float *out_q /* may be NULL */,
                    float *out_dqda /* may be NULL */, float *out_stats /* may be NULL */, void *stream);

/* ---- wide device-resident MlpPolicy (gym_xarm_amd/csrc/xarm_acw_core.h, xarm_k_acw.hip): xarm_policy_act's contract for
 * gym_xarm_amd/train.py's ActorCritic(net_arch, activation) with equal-width towers of n_hidden = 2 or 3 hidden layers of hidden = 64,
 * 128, 192 or 256 units, tanh or ReLU (XARM_SACW_TANH / XARM_SACW_RELU).  Rows, stats, calls, the noise and the four outputs mean what
 * they mean in xarm_policy_act, except that EVERY output may be NULL (a NULL out_value skips the value tower).  A tower is 2 (n_hidden + 1)
 * pointers W1, b1, ..., W_out, b_out (nn.Linear's [out, in] layout) in arrays of eight, the unused tail ignored.  The forward runs layer
 * by layer on xarm_sacw's f32 MFMA GEMM kernel with the activations in `workspace`: one launch writes the row observation |
 * achieved_goal | desired_goal (normalised when stats is set) there, n_hidden + 1 launches run both towers, one launch per row draws the
 * noise and writes the outputs, and a stochastic call ends with the one-thread launch that advances `calls` - n_hidden + 3 (+ 1) launches
 * for every row count.  Every dot product is a float32 fmaf chain from the bias over k ascending (an odd K padded with one zero operand):
 * a row's result depends on that row, the weights, seed, row_offset + row and *calls alone.  No allocation, no host read, no atomics, no
 * side stream; num_rows == 0 launches nothing. */
typedef struct xarm_acw_layout {
    int32_t num_rows;
    int32_t obs_dim;
    int32_t goal_dim;           /* 0: `obs` is the whole row */
    int32_t act_dim;            /* 1 .. XARM_POLICY_MAX_ACT */
    int32_t hidden;             /* 64, 128, 192 or 256 */
    int32_t n_hidden;           /* 2 or 3 */
    int32_t activation;         /* XARM_SACW_TANH or XARM_SACW_RELU */
    int64_t row_offset;         /* global index of row 0 (>= 0) */
} xarm_acw_layout;              /* 40 bytes (4 bytes of padding before row_offset) */
typedef struct xarm_acw_weights {
    const float *pi[2 * (XARM_SACW_MAX_LAYERS + 1)];        /* W1 [H, D], b1 [H], W2 [H, H], b2 [H], (W3, b3,) W_out [A, H], b_out [A] */
    const float *vf[2 * (XARM_SACW_MAX_LAYERS + 1)];        /* ..., W_out [1, H], b_out [1]; read only when out_value is set */
    const float *log_std;       /* [A] */
} xarm_acw_weights;             /* 17 device pointers */
/* *bytes = size of xarm_acw_act's `workspace` for this layout: (D + 2 n_hidden hidden + A + 1) floats per row, each part rounded up to
 * 16 bytes.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_acw_workspace_bytes(const xarm_acw_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: NULL layout / params / weights, num_rows < 0, obs_dim < 1, goal_dim < 0, D > XARM_POLICY_MAX_DIM, act_dim outside
 * [1, XARM_POLICY_MAX_ACT], hidden outside {64, 128, 192, 256}, n_hidden outside {2, 3}, activation outside {XARM_SACW_TANH,
 * XARM_SACW_RELU}, row_offset < 0, with stats an eps that is not finite and > 0 or a clip_obs <= 0, or with num_rows > 0 a NULL policy
 * tensor, log_std or obs, a NULL achieved_goal / desired_goal with goal_dim > 0, a NULL value tensor with out_value set, a tensor from
 * b1 to W_out (of a tower that is read) that is not 16-byte aligned, a NULL or not 16-byte aligned workspace, a NULL calls with
 * deterministic == 0. */
int xarm_acw_act(const xarm_acw_layout *layout, const xarm_policy_params *params, const xarm_acw_weights *weights,
                 const double *stats /* may be NULL */, int64_t *calls_i64, const float *obs, const float *achieved_goal,
                 const float *desired_goal, void *workspace, float *out_action /* may be NULL */, float *out_env_action /* may be NULL */,
                 float *out_logp /* may be NULL */, float *out_value /* may be NULL */, void *stream);

/* ---- wide device-resident PPO update (gym_xarm_amd/csrc/xarm_ppow_core.h, xarm_k_ppow.hip): xarm_ppo_update for the towers
 * of xarm_acw_act.  Arguments and every meaning are xarm_ppo_update's - obs [T, E, D], action, reward, done, use (may be NULL), last_obs,
 * old_logp (may be NULL), perm int32 [n_epochs, N], out_adv / out_returns [T, E], out_grad [P] (step 0, before the clip), out_stats
 * [S, 8] - with the layout naming hidden, n_hidden and activation and the weights, exp_avg and exp_avg_sq as three xarm_acw_weights.
 * out_grad's flat order: pi's 2 (n_hidden + 1) tensors, vf's, log_std.  With L = n_hidden, B = min(batch_size, N), M = ceil(N / B),
 * S = n_epochs M and c = M + ceil(E / B) (the call-start forward runs the rollout in M chunks of at most B rows and last_obs in
 * launches of its own) a call is c (L + 1) + 2 + S (2 L + 6) launches: the workspace grows with B, not with N, apart from N (A + 4) + E
 * floats of per-row results.  No allocation, no host read, no atomics, no side stream; sums run in a fixed order (xarm_sacw's for the
 * weight gradients, 256 float64 partials added in order for sums over rows): the same inputs and perm give the same bits.
 * xarm_ppow_update_opt takes xarm_ppo_update_opt's options with the same meaning: with clip_range_vf the gather carries the call-start
 * value as one more column; with target_kl every launch of a stopped step returns after one read of the flag.  Both off: the same launches,
 * grids and bits.
 * Out of scope: unequal widths, a shared trunk.  num_envs == 0 launches nothing. */
typedef struct xarm_ppow_layout {
    int32_t num_envs;           /* E >= 0 */
    int32_t n_steps;            /* T >= 1, T E < 2^31 */
    int32_t obs_dim;            /* D: 1 .. XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_POLICY_MAX_ACT */
    int32_t hidden;             /* 64, 128, 192 or 256 */
    int32_t n_hidden;           /* 2 or 3 */
    int32_t activation;         /* XARM_SACW_TANH or XARM_SACW_RELU */
    int32_t n_epochs;           /* >= 1 */
    int32_t batch_size;         /* >= 1; n_epochs ceil(T E / batch_size) <= 4096 */
} xarm_ppow_layout;             /* 36 bytes */
/* *bytes = size of `workspace` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_ppow_workspace_bytes(const xarm_ppow_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: what xarm_ppo_update refuses, with hidden outside {64, 128, 192, 256}, n_hidden outside {2, 3} or activation outside
 * {XARM_SACW_TANH, XARM_SACW_RELU} in place of hidden != 64; with num_envs > 0 a NULL tensor of either tower, of log_std or of the two
 * states, a weight tensor from b1 to W_out that is not 16-byte aligned, a NULL or not 16-byte aligned workspace. */
int xarm_ppow_update(const xarm_ppow_layout *layout, const xarm_ppo_params *params, const xarm_acw_weights *weights,
                     const xarm_acw_weights *exp_avg, const xarm_acw_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                     const float *action, const float *reward, const float *done, const float *use /* may be NULL */,
                     const float *last_obs, const float *old_logp /* may be NULL */, const int32_t *perm, void *workspace,
                     float *out_adv /* may be NULL */, float *out_returns /* may be NULL */, float *out_grad /* may be NULL */,
                     float *out_stats /* may be NULL */, void *stream);
int xarm_ppow_update_opt(const xarm_ppow_layout *layout, const xarm_ppo_params *params, const xarm_acw_weights *weights,
                         const xarm_acw_weights *exp_avg, const xarm_acw_weights *exp_avg_sq, int64_t *step_i64, const float *obs,
                         const float *action, const float *reward, const float *done, const float *use /* may be NULL */,
                         const float *last_obs, const float *old_logp /* may be NULL */, const int32_t *perm, void *workspace,
                         float *out_adv /* may be NULL */, float *out_returns /* may be NULL */, float *out_grad /* may be NULL */,
                         float *out_stats /* may be NULL */, const xarm_ppo_options *options /* NULL = none */, void *stream);

/* ---- wide device-resident A2C update (gym_xarm_amd/csrc/xarm_a2cw_core.h, xarm_k_a2cw.hip): xarm_a2c_update for the towers
 * of xarm_acw_act.  Arguments and every meaning are xarm_a2c_update's - obs [T, E, D], action, reward, done, use (may be NULL), last_obs,
 * out_returns [T, E], out_grad [P] (before the clip), out_stats [8] = policy_loss, value_loss, entropy, grad_norm, n_use, 0, 0, 0 - with
 * the layout naming hidden, n_hidden and activation and the weights and square_avg as two xarm_acw_weights (READ AND WRITTEN in place).
 * Flat order of out_grad and square_avg: pi's 2 (n_hidden + 1) tensors, vf's, log_std.  It is xarm_ppow_update's chain with one optimiser
 * step over all N = T E rows in their stored order: with L = n_hidden, L + 1 forward launches of vf over last_obs, one launch for the
 * returns, L + 1 forward launches of both towers over the rollout (read from obs in place), the head on min(64, ceil(N / 256)) workgroups,
 * L delta launches, one weight-gradient launch, reduce and apply - 3 L + 7 launches for every row count.  The workspace holds every
 * layer's activations and deltas of all N rows (4 L N hidden floats and N (2 act_dim + 3) + E of per-row results, at most 16 gradient
 * partials, the head's records) and nothing between calls.  No allocation, no host read, no atomics, no side stream; sums run in a fixed
 * order (xarm_sacw's for the weight gradients; for sums over rows 256 float64 partials per head workgroup added in thread order, the
 * workgroups' records in workgroup order): the same inputs give the same bits.  Out of scope: unequal widths, a shared trunk, chunked
 * batches.  num_envs == 0 launches nothing. */
typedef struct xarm_a2cw_layout {
    int32_t num_envs;           /* E >= 0 */
    int32_t n_steps;            /* T >= 1, T E < 2^31 */
    int32_t obs_dim;            /* D: 1 .. XARM_POLICY_MAX_DIM */
    int32_t act_dim;            /* 1 .. XARM_POLICY_MAX_ACT */
    int32_t hidden;             /* 64, 128, 192 or 256 */
    int32_t n_hidden;           /* 2 or 3 */
    int32_t activation;         /* XARM_SACW_TANH or XARM_SACW_RELU */
} xarm_a2cw_layout;             /* 28 bytes */
/* *bytes = size of `workspace` for this layout.  XARM_E_INVALID: NULL argument or unusable layout (below). */
int xarm_a2cw_workspace_bytes(const xarm_a2cw_layout *layout, int64_t *bytes);
/* XARM_E_INVALID: what xarm_a2c_update refuses, with hidden outside {64, 128, 192, 256}, n_hidden outside {2, 3} or activation outside
 * {XARM_SACW_TANH, XARM_SACW_RELU} in place of hidden != 64; with num_envs > 0 a NULL tensor of either tower, of log_std or of square_avg,
 * a weight tensor from b1 to W_out that is not 16-byte aligned, a NULL or not 16-byte aligned workspace. */
int xarm_a2cw_update(const xarm_a2cw_layout *layout, const xarm_a2c_params *params, const xarm_acw_weights *weights,
                     const xarm_acw_weights *square_avg, const float *obs, const float *action, const float *reward, const float *done,
                     const float *use /* may be NULL */, const float *last_obs, void *workspace, float *out_returns /* may be NULL */,
                     float *out_grad /* may be NULL */, float *out_stats /* may be NULL */, void *stream);

/* ---- a device shuffle for the PPO update's `perm` (gym_xarm_amd/csrc/xarm_rollout_core.h, xarm_k_rollout.hip).  Like
 * the calls above it needs no env handle: everything is caller-owned DEVICE memory, the launches go to `stream` on the caller's current
 * device, the messages of XARM_E_INVALID go to xarm_last_error(NULL).  The call does not allocate, synchronise, read device memory from
 * the host or use an atomic: the same inputs give the same bits, and it can be captured in a graph. */
/* perm_i32 [n_epochs, N] <- n_epochs independent pseudo-random permutations of [0, N), one thread per entry, no sort, no workspace:
 * entry i of epoch ep is i enciphered by a keyed bijection of [0, 2^b), b = max(8, ceil(log2 N)), again and again until the value is
 * below N (cycle walking).  The bijection is an alternating unbalanced Feistel network of 8 rounds over the low floor(b / 2) and the
 * high ceil(b / 2) bits whose round function is the first word of Philox(seed; the other half, round | ep << 8, low word of calls,
 * 0x5045524D + high word of calls), masked to the width of the half it is x-ored into.  N == 1 writes 0, N == 0 launches nothing.
 * *calls_i64 (int64 [1], zero at the start) is read by every thread and advanced by one behind the fill, on the device, so the replays
 * of a captured graph draw a fresh shuffle each.  Two launches.  XARM_E_INVALID: N outside [0, 2^31), n_epochs outside [1, 255], a NULL
 * pointer with N > 0. */
int xarm_perm_fill(int32_t *perm_i32, int32_t n_epochs, int64_t N, uint64_t seed, int64_t *calls_i64, void *stream);

const char *xarm_last_error(const xarm_handle *h);
const char *xarm_version(void);

#ifdef __cplusplus
}
#endif
#endif
