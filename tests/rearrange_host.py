"""ctypes view of tests/hostbuild_rearrange (g++ build of the cube core csrc/xarm_stack_core.h for the scene of
csrc/xarm_rearrange_core.h, float64 and float32) - CPU-side tests only.  Rows are float64 state rows [E, 160] in the layout of
the header comment of xarm_stack_core.h with N = 4.
reset_reference / step_auto are what the device's reset and auto-resetting step are held to: the reset spelled out in NumPy
(teleport, the draws through the oracle's Philox, placement, goals) around one bare tick of the core, so that neither the draw
keying nor the reset sequence rests on lane_reset, and the reset's conditioning can be probed (perturb)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_rearrange")
STATE_DIM, OBS_DIM, GOAL_DIM = 160, 68, 12
# state fields (xra::Rearrange4::K_*)
Q, QD, QT, BP, BQ, BV, BW, GOAL, LT, LP, STEPS, EPISODE = 0, 18, 36, 54, 66, 82, 94, 106, 118, 150, 158, 159
# StackTower's (xs::Tower3::K_*)
S_BP, S_BQ, S_BV, S_BW, S_GOAL, S_LT, S_LP, S_STEPS, S_EPISODE = 54, 63, 75, 84, 93, 102, 126, 134, 135
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "librearrange_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "rearrange_host.cpp"), os.path.join(ROOT, "tests", "hostbuild", "cube_pair_host.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-pthread", "-o", tmp, srcs[0]])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp, i64, u64, i32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int
    L.ra_dims.argtypes = [vp]
    L.ra_init.argtypes = [i32, u64, i64, i32, i64, vp]
    L.ra_step.argtypes = [i32, u64, i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ra_reset.argtypes = [i32, u64, i64, i32, i64, vp, vp, vp, vp, vp, vp]
    L.ra_tick.argtypes = [i32, i64, vp, vp]
    L.ra_arm_obs.argtypes = [i64, vp, vp]
    L.ra_compute_reward.argtypes = [i32, vp, vp, i64, vp]
    L.ra_class_order.argtypes = [vp, i64, i32, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data


def init(E, f32=0, seed=0, off=0, rt=0):
    st = np.zeros((E, STATE_DIM))
    lib().ra_init(f32, seed, off, rt, E, _p(st))
    return st


WORKERS = 4      # row blocks of a large batch run side by side (each call runs an env's two lanes as two threads: 8 threads)


def _blocks(E, call):
    """call(lo, hi) over the rows in up to WORKERS contiguous blocks, concurrently (ctypes releases the GIL); the rows are
    independent, so the split changes no number"""
    n = min(WORKERS, max(1, E // 16))
    edges = [E * i // n for i in range(n + 1)]
    if n == 1:
        call(0, E)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(n) as pool:
        for f in [pool.submit(call, lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]:
            f.result()


def step(state, actions, f32=0, seed=0, off=0, rt=0):
    """-> state, obs, ag, dg, reward, done, success, class key (row-set class of the last substep)"""
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    E = st.shape[0]
    act = np.ascontiguousarray(actions, dtype=np.float64)
    obs, ag, dg = np.zeros((E, OBS_DIM)), np.zeros((E, GOAL_DIM)), np.zeros((E, GOAL_DIM))
    rew, done, succ, key = np.zeros(E), np.zeros(E, np.uint8), np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    L = lib()
    _blocks(E, lambda a, b: L.ra_step(f32, seed, off + a, rt, b - a, _p(st[a:]), _p(act[a:]), _p(obs[a:]), _p(ag[a:]), _p(dg[a:]), _p(rew[a:]),
                                      _p(done[a:]), _p(succ[a:]), _p(key[a:])))
    return st, obs, ag, dg, rew, done, succ, key


def reset(state, mask=None, f32=0, seed=0, off=0, rt=0):
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    E = st.shape[0]
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    obs, ag, dg, key = np.zeros((E, OBS_DIM)), np.zeros((E, GOAL_DIM)), np.zeros((E, GOAL_DIM)), np.zeros(E, np.uint8)
    lib().ra_reset(f32, seed, off, rt, E, _p(st), None if m is None else _p(m), _p(obs), _p(ag), _p(dg), _p(key))
    return st, obs, ag, dg, key


def tick(state, f32=0):
    """one bare tick (15 substeps towards the stored motor targets) of every row -> state, class key"""
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    key = np.zeros(st.shape[0], np.uint8)
    L = lib()
    _blocks(st.shape[0], lambda a, b: L.ra_tick(f32, b - a, _p(st[a:]), _p(key[a:])))
    return st, key


def outputs(state):
    """obs, ag, dg of state rows: the cube columns copied, the 16 arm entries from the core's arm_obs (float64)"""
    st = np.ascontiguousarray(state, dtype=np.float64)
    E = st.shape[0]
    arm = np.zeros((E, 16))
    lib().ra_arm_obs(E, _p(st), _p(arm))
    obs = np.concatenate([st[:, BP:BP + 12], st[:, BQ:BQ + 16], st[:, BV:BV + 12], st[:, BW:BW + 12], arm], axis=1)
    return obs, st[:, BP:BP + 12].copy(), st[:, GOAL:GOAL + 12].copy()


_scene = None


def scene():
    """joint_init_pos and the spawn / goal ranges, from the model JSON (not from a header)"""
    global _scene
    if _scene is None:
        with open(os.path.join(ROOT, "gym_xarm_amd", "model", "xarm7_pd.json")) as f:
            js = json.load(f)
        ra = js["rearrange"]
        _scene = dict(q0=np.array(js["stack_tower"]["joint_init_pos"], dtype=np.float64), z=float(js["stack_tower"]["height_offset"]),
                      **{k: np.array(ra[k], dtype=np.float64) for k in ("obj_low", "obj_high", "goal_low", "goal_high")})
    return _scene


def uniforms(seed, gid, episode):
    """the 16 uniforms of env `gid`'s reset into `episode`: four Philox blocks keyed (gid low word, gid high word, episode, block)"""
    from oracle import oracle as O
    gid = int(gid)
    return np.array([(x >> 8) / 2.0 ** 24 for b in range(4) for x in O.philox(int(seed), gid & 0xffffffff, gid >> 32, int(episode), b)])


def drawn(seed, off, episodes, envs=None):
    """-> cube xy [n, 4, 2], goal xy [n, 4, 2] as drawn for envs off + envs[i] (default: i) entering episodes[i]"""
    sc = scene()
    envs = range(len(episodes)) if envs is None else envs
    u = np.array([uniforms(seed, off + int(e), ep) for e, ep in zip(envs, episodes)])
    cube = sc["obj_low"] + u[:, 0:8].reshape(-1, 4, 2) * (sc["obj_high"] - sc["obj_low"])
    goal = sc["goal_low"] + u[:, 8:16].reshape(-1, 4, 2) * (sc["goal_high"] - sc["goal_low"])
    return cube, goal


def reset_reference(state, mask=None, seed=0, off=0, perturb=None):
    """The reset spelled out in NumPy around one bare tick of the float64 core: teleport (qt kept), the draws through the oracle's
    Philox, cubes placed, [perturb: a Generator; +-1e-6 on q, qt and the cube positions], tick, goals, steps = 0, episode + 1.
    -> state, obs, ag, dg, key; rows outside the mask keep their state, their outputs and key are 0 (as reset())"""
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    E = st.shape[0]
    m = np.ones(E, bool) if mask is None else np.asarray(mask).astype(bool)
    idx = np.where(m)[0]
    obs, ag, dg, key = np.zeros((E, OBS_DIM)), np.zeros((E, GOAL_DIM)), np.zeros((E, GOAL_DIM)), np.zeros(E, np.uint8)
    if idx.size == 0:
        return st, obs, ag, dg, key
    sc = scene()
    r = st[idx]
    episode = r[:, EPISODE].astype(np.int64) + 1
    cube, goal = drawn(seed, off, episode, idx)
    r[:, Q:Q + 18] = np.tile(sc["q0"], 2)
    r[:, QD:QD + 18] = 0
    bp = np.concatenate([cube, np.full((idx.size, 4, 1), sc["z"])], axis=2)
    r[:, BP:BP + 12] = bp.reshape(-1, 12)
    r[:, BQ:BQ + 16] = [0, 0, 0, 1] * 4
    r[:, BV:BV + 24] = 0
    r[:, LT:LP + 8] = 0
    if perturb is not None:
        cols = np.r_[Q:Q + 18, QT:QT + 18, BP:BP + 12]
        r[:, cols] += perturb.uniform(-1e-6, 1e-6, (idx.size, cols.size))
    r, k = tick(r)
    r[:, GOAL:GOAL + 12] = np.concatenate([goal, np.full((idx.size, 4, 1), sc["z"])], axis=2).reshape(-1, 12)
    r[:, STEPS] = 0
    r[:, EPISODE] = episode
    st[idx] = r
    obs[idx], ag[idx], dg[idx] = outputs(r)
    key[idx] = k
    return st, obs, ag, dg, key


RESET_FIELDS = np.r_[Q:Q + 18, BP:BP + 12, BQ:BQ + 16, BV:BV + 24]   # what a reset comparison looks at in the state (+ obs)


def reset_sens(state, ref, mask=None, seed=0, off=0, draws=2, rng_seed=0):
    """per env: the largest response of reset_reference's compared state fields and observation to `draws` +-1e-6
    perturbations of the pre-tick state; ref = reset_reference's own (state, obs, ...) of the same call"""
    sens = np.zeros(ref[0].shape[0])
    for j in range(draws):
        p = reset_reference(state, mask, seed, off, perturb=np.random.default_rng(1000 * rng_seed + j))
        sens = np.maximum(sens, np.maximum(np.abs(p[0][:, RESET_FIELDS] - ref[0][:, RESET_FIELDS]).max(axis=1), np.abs(p[1] - ref[1]).max(axis=1)))
    return sens


def step_auto(state, actions, seed=0, off=0, rt=0, perturb=None):
    """what an auto-resetting step call returns: step(), then reset_reference of the envs whose done is set.
    -> dict: state (after the call), obs / ag / dg (post-reset for the envs that ended, the step's for the rest), term (the
    step's own obs), rew, done, succ, key, and step = the plain step's tuple.  perturb reaches the resets only."""
    s = step(state, actions, f32=0, seed=seed, off=off, rt=rt)
    done = s[5].astype(bool)
    r = reset_reference(s[0], done, seed, off, perturb)
    pick = done[:, None]
    return dict(state=r[0], obs=np.where(pick, r[1], s[1]), ag=np.where(pick, r[2], s[2]), dg=np.where(pick, r[3], s[3]), term=s[1],
                rew=s[4], done=s[5], succ=s[6], key=np.where(done, r[4], s[7]), step=s, reset=r)


def compute_reward(ag, g, rt):
    a, b = np.ascontiguousarray(ag, dtype=np.float32).reshape(-1, 12), np.ascontiguousarray(g, dtype=np.float32).reshape(-1, 12)
    out = np.zeros(a.shape[0], np.float32)
    lib().ra_compute_reward(rt, _p(a), _p(b), a.shape[0], _p(out))
    return out


def class_order(key, group=32):
    k = np.ascontiguousarray(key, dtype=np.uint8)
    order = np.zeros(k.size, np.int32)
    r = lib().ra_class_order(_p(k), k.size, group, _p(order))
    assert r >= 0, "not a permutation"
    return order, bool(r)


def live_cubes(parked):
    return [c for c in range(4) if c != parked]


def from_stack(st_rows, parked, park_xy=(0.0, 0.45)):
    """Rearrange rows holding a StackTower state [E, 136]: its three cubes become the Rearrange cubes other than `parked`,
    in order; cube `parked` rests on the table at park_xy, its goal where it lies"""
    s3 = np.asarray(st_rows, dtype=np.float64)
    E = s3.shape[0]
    r = np.zeros((E, STATE_DIM))
    r[:, 0:54] = s3[:, 0:54]
    for j, c in enumerate(live_cubes(parked)):
        r[:, BP + 3 * c:BP + 3 * c + 3] = s3[:, S_BP + 3 * j:S_BP + 3 * j + 3]
        r[:, BQ + 4 * c:BQ + 4 * c + 4] = s3[:, S_BQ + 4 * j:S_BQ + 4 * j + 4]
        r[:, BV + 3 * c:BV + 3 * c + 3] = s3[:, S_BV + 3 * j:S_BV + 3 * j + 3]
        r[:, BW + 3 * c:BW + 3 * c + 3] = s3[:, S_BW + 3 * j:S_BW + 3 * j + 3]
        r[:, GOAL + 3 * c:GOAL + 3 * c + 3] = s3[:, S_GOAL + 3 * j:S_GOAL + 3 * j + 3]
        r[:, LT + 8 * c:LT + 8 * c + 8] = s3[:, S_LT + 8 * j:S_LT + 8 * j + 8]
    r[:, BP + 3 * parked:BP + 3 * parked + 3] = [park_xy[0], park_xy[1], 0.025]
    r[:, BQ + 4 * parked + 3] = 1.0
    r[:, GOAL + 3 * parked:GOAL + 3 * parked + 3] = [park_xy[0], park_xy[1], 0.025]
    r[:, LP:LP + 8] = s3[:, S_LP:S_LP + 8]
    r[:, STEPS], r[:, EPISODE] = s3[:, S_STEPS], s3[:, S_EPISODE]
    return r


def to_stack(rows, parked, like):
    """the StackTower view of Rearrange rows (cube `parked` dropped); `like` supplies the StackTower goals"""
    r = np.asarray(rows, dtype=np.float64)
    s3 = np.array(like, dtype=np.float64, copy=True)
    s3[:, 0:54] = r[:, 0:54]
    for j, c in enumerate(live_cubes(parked)):
        s3[:, S_BP + 3 * j:S_BP + 3 * j + 3] = r[:, BP + 3 * c:BP + 3 * c + 3]
        s3[:, S_BQ + 4 * j:S_BQ + 4 * j + 4] = r[:, BQ + 4 * c:BQ + 4 * c + 4]
        s3[:, S_BV + 3 * j:S_BV + 3 * j + 3] = r[:, BV + 3 * c:BV + 3 * c + 3]
        s3[:, S_BW + 3 * j:S_BW + 3 * j + 3] = r[:, BW + 3 * c:BW + 3 * c + 3]
        s3[:, S_LT + 8 * j:S_LT + 8 * j + 8] = r[:, LT + 8 * c:LT + 8 * c + 8]
    s3[:, S_LP:S_LP + 8] = r[:, LP:LP + 8]
    s3[:, S_STEPS], s3[:, S_EPISODE] = r[:, STEPS], r[:, EPISODE]
    return s3
