"""ctypes view of tests/hostbuild_policy (g++ -ffp-contract=off build of csrc/xarm_policy_core.h) - CPU-side tests only - with
the weight / input cases, the float64 NumPy restatement of ActorCritic's forward and of the noise (from the same Philox words,
generated here in NumPy) and the float32 NumPy evaluation of the noise formulas that the host and GPU policy tests share."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_policy")
WIDTHS = ((8, 3), (24, 3), (29, 0), (68, 12), (96, 0))     # Reach, PickAndPlace, an odd flat row, Rearrange, the maximum
ACT_DIMS = (1, 4, 8, 16)
SIZES = (1, 31, 32, 33, 63, 64, 65, 1000)
ROWS = 1000
GXX_FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_lib = None
_cases = {}


def gxx_flags():
    """std::fmaf as the hardware instruction where the CPU has one (same bits as the library routine, which is ~40x slower)"""
    try:
        fma = " fma " in open("/proc/cpuinfo").read()
    except OSError:
        fma = False
    return GXX_FLAGS + (["-mfma"] if fma else [])


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "policy_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libpolicy_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ph_act.argtypes = [vp] * 12
    for f in (L.ph_tanh, L.ph_exp, L.ph_log):
        f.argtypes = [vp, vp, C.c_int64]
    L.ph_sincos_turn.argtypes = [vp, vp, vp, C.c_int64]
    L.ph_kord.argtypes = [vp]
    L.ph_philox_tag.restype = C.c_uint32
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def aligned(a):
    """a float32 copy of `a` at a 16-byte aligned address (the call reads b1, W2, b2 and W3 in 16-byte pieces)"""
    a = np.ascontiguousarray(a, np.float32)
    raw = np.empty(a.size * 4 + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + a.size * 4].view(np.float32).reshape(a.shape)
    out[...] = a
    return out


NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w3", "pi_b3", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_w3", "vf_b3", "log_std")


def model_params(model):
    m = model
    return (m.pi[0].weight, m.pi[0].bias, m.pi[2].weight, m.pi[2].bias, m.pi[4].weight, m.pi[4].bias,
            m.vf[0].weight, m.vf[0].bias, m.vf[2].weight, m.vf[2].bias, m.vf[4].weight, m.vf[4].bias, m.log_std)


def weights_of(model):
    """the model's 13 parameter tensors as aligned NumPy arrays, by the ABI's field names"""
    return {k: aligned(t.detach().cpu().numpy()) for k, t in zip(NAMES, model_params(model))}


def split(rows, obs_dim, goal_dim):
    """a [E, D] row set as the call's three inputs (None for the goal parts of a flat row)"""
    c = np.ascontiguousarray
    if goal_dim == 0:
        return [c(rows), None, None]
    return [c(rows[:, :obs_dim]), c(rows[:, obs_dim:obs_dim + goal_dim]), c(rows[:, obs_dim + goal_dim:])]


def host_act(w, rows, obs_dim, goal_dim, stats=None, deterministic=False, seed=0, row_offset=0, calls=None, logp=True, value=True,
             clip_obs=10.0, eps=1e-8):
    """one call of the host build; the outputs are filled with NaN first.  calls: int64 [1], advanced by a stochastic call."""
    from gym_xarm_amd import _native
    E, A = rows.shape[0], w["log_std"].shape[0]
    layout = _native.XarmPolicyLayout(E, obs_dim, goal_dim, A, 64, row_offset)
    params = _native.XarmPolicyParams(seed, clip_obs, eps, int(deterministic))
    ws = _native.XarmPolicyWeights(*[w[k].ctypes.data for k in NAMES])
    calls = np.zeros(1, np.int64) if calls is None else calls
    out = {"action": np.full((E, A), np.nan, np.float32), "env_action": np.full((E, A), np.nan, np.float32),
           "logp": np.full(E, np.nan, np.float32) if logp else None, "value": np.full(E, np.nan, np.float32) if value else None}
    parts = split(rows, obs_dim, goal_dim)                 # held until the call has returned
    rc = lib().ph_act(C.byref(layout), C.byref(params), C.byref(ws), _p(stats), _p(calls), *[_p(x) for x in parts],
                      _p(out["action"]), _p(out["env_action"]), _p(out["logp"]), _p(out["value"]))
    assert rc == 0
    return out


def make_model(D, A, scale=1.0, seed=0):
    """ActorCritic's own initialisation under a fixed seed, every weight and bias of the towers multiplied by `scale` (4: the
    tanh saturates), log_std uniform on [-2, 0.5]"""
    from gym_xarm_amd.train import ActorCritic
    g = torch.random.get_rng_state()
    torch.manual_seed(4321 + 97 * D + A + seed)
    model = ActorCritic(D, A)
    with torch.no_grad():
        for t in model_params(model)[:12]:
            t.mul_(scale)
        model.log_std.copy_(torch.rand(A) * 2.5 - 2.0)
    torch.random.set_rng_state(g)
    return model


def normalise(rows, stats, clip=10.0, eps=1e-8):
    """the frozen-statistics normalisation: float64, clamp, one rounding to float32"""
    D = rows.shape[1]
    return np.clip((rows.astype(np.float64) - stats[:D]) / np.sqrt(stats[D:2 * D] + eps), -clip, clip).astype(np.float32)


def ref64(w, x):
    """ActorCritic's forward restated in float64 NumPy on float32 inputs x [E, D]: (mean [E, A], value [E])"""
    f = lambda k: w[k].astype(np.float64)

    def tower(p):
        h = np.tanh(x.astype(np.float64) @ f(p + "_w1").T + f(p + "_b1"))
        h = np.tanh(h @ f(p + "_w2").T + f(p + "_b2"))
        return h @ f(p + "_w3").T + f(p + "_b3")
    return tower("pi"), tower("vf")[:, 0]


def case(od, gd, A, scale):
    """weights, the 1000 input rows in [-10, 10], the float64 restatement and torch's float32 ActorCritic on them, and the host
    build's deterministic outputs.  Computed once per case and only read."""
    key = (od, gd, A, scale)
    if key in _cases:
        return _cases[key]
    D = od + 2 * gd
    model = make_model(D, A, scale)
    w = weights_of(model)
    rows = np.random.RandomState(11 * D + A).uniform(-10, 10, (ROWS, D)).astype(np.float32)
    mean64, value64 = ref64(w, rows)
    with torch.no_grad():
        x = torch.from_numpy(rows)
        mean32, value32 = model.pi(x).numpy(), model.value(x).numpy()
    det = host_act(w, rows, od, gd, deterministic=True)
    _cases[key] = dict(model=model, w=w, rows=rows, mean64=mean64, value64=value64, mean32=mean32, value32=value32, det=det, D=D)
    return _cases[key]


# ---- the noise: Philox4x32-10 in NumPy (csrc/xarm_core.h xk::philox), Box-Muller in float64 and in float32
def philox(seed, c0, c1, c2, c3):
    """words [..., 4] for counter arrays (broadcast), uint32 arithmetic carried in uint64"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) & M for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n1 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M
        n2, n3 = (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def noise_words(seed, rows, calls, A):
    """the Philox words behind z [len(rows), A]: [E, blocks, 4]; rows are GLOBAL row indices"""
    rows = np.asarray(rows, np.uint64)[:, None]
    b = np.arange((A + 3) // 4, dtype=np.uint64)[None, :]
    tag = np.uint64(lib().ph_philox_tag())
    return philox(seed, rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), np.uint64(calls & 0xFFFFFFFF),
                  tag + b + np.uint64(((calls >> 32) & 0xFFFFFFFF) << 2))


def box_muller(words, dtype):
    """z [E, 4 blocks] from words [E, blocks, 4] with every operation in `dtype`: u = ((w >> 8) + 1) 2^-24, r = sqrt(-2 ln u1),
    z = r cos(2 pi u2), r sin(2 pi u2)"""
    t = dtype
    u = ((words >> np.uint32(8)).astype(np.int64) + 1).astype(t) * t(2.0 ** -24)
    out = np.empty(words.shape, t)
    for k in (0, 2):
        r = np.sqrt(t(-2.0) * np.log(u[..., k]))
        th = t(2.0 * np.pi) * u[..., k + 1]
        out[..., k], out[..., k + 1] = r * np.cos(th), r * np.sin(th)
        assert out.dtype == t and r.dtype == t and th.dtype == t
    return out.reshape(words.shape[0], -1)


def ulp32(x):
    """one float32 unit in the last place at the magnitude of x"""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def bits(x):
    return np.ascontiguousarray(x).tobytes()
