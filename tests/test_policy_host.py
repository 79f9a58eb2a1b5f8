"""The device-resident MlpPolicy's core (gym_xarm_amd/csrc/xarm_policy_core.h) on the CPU: the g++ build (tests/policy_host.py)
against a float64 NumPy restatement of ActorCritic's forward with torch's own float32 ActorCritic as the yardstick, the noise
against a float64 restatement from the same Philox words with a float32 NumPy evaluation as the yardstick, the noise's
statistics, the identities of the outputs, the argument checks of the C-ABI entry point through the real library (no device
needed), and an address / undefined-behaviour sanitizer run of the host core as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_host as PH

SCALES = (1.0, 4.0)


def forward_tolerance(c):
    """per quantity: twice the largest deviation of torch's float32 ActorCritic (CPU) from the float64 restatement on the case's
    1000 rows, plus one float32 ulp at the quantity's largest magnitude.  The yardstick is the torch class, never the core."""
    dev = {"mean": float(np.abs(c["mean32"] - c["mean64"]).max()), "value": float(np.abs(c["value32"] - c["value64"]).max())}
    tol = {"mean": 2.0 * dev["mean"] + float(PH.ulp32(np.abs(c["mean64"]).max())),
           "value": 2.0 * dev["value"] + float(PH.ulp32(np.abs(c["value64"]).max()))}
    return dev, tol


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("A", PH.ACT_DIMS)
@pytest.mark.parametrize("od,gd", PH.WIDTHS)
def test_forward_against_float64_with_torch_as_the_yardstick(od, gd, A, scale):
    """mean, value and the deterministic action on 1000 rows in [-10, 10]; every smaller batch is the same rows bit for bit.
    Measured (largest over the cases, mean / value): host core - float64 3.7e-7 / 3.5e-7 where torch - float64 is 3.8e-7 / 2.5e-7 at
    the initialisation's own scale, 9.7e-6 / 5.7e-6 against 6.8e-6 / 5.4e-6 with the weights x 4."""
    c = PH.case(od, gd, A, scale)
    dev, tol = forward_tolerance(c)
    det = c["det"]
    host = {"mean": float(np.abs(det["action"] - c["mean64"]).max()), "value": float(np.abs(det["value"] - c["value64"]).max())}
    print("D %d A %d x%g: host core - float64 %s; torch float32 - float64 %s; tolerance %s" % (c["D"], A, scale, host, dev, tol))
    assert host["mean"] <= tol["mean"] and host["value"] <= tol["value"]
    assert PH.bits(det["env_action"]) == PH.bits(np.clip(det["action"], -1, 1))
    for E in PH.SIZES:
        out = PH.host_act(c["w"], c["rows"][:E], od, gd, deterministic=True)
        for k in ("action", "env_action", "logp", "value"):
            assert PH.bits(out[k]) == PH.bits(det[k][:E]), (E, k)


@pytest.mark.parametrize("A", PH.ACT_DIMS)
@pytest.mark.parametrize("od,gd", PH.WIDTHS[:2])
def test_frozen_statistics_normalise_the_row_before_the_network(od, gd, A):
    """stats set: the call on raw rows equals, bit for bit, the call on the rows normalised in float64 NumPy"""
    c = PH.case(od, gd, A, 1.0)
    D = c["D"]
    rng = np.random.RandomState(5)
    stats = np.concatenate([rng.uniform(-1, 1, D), rng.uniform(0.05, 4, D), [0.0, 1.0, 1000.0, 1000.0]])
    raw = c["rows"][:65]                                     # up to 10 / sqrt(0.05) standard deviations out: some columns clip
    a = PH.host_act(c["w"], raw, od, gd, stats=stats, seed=3)
    b = PH.host_act(c["w"], PH.normalise(raw, stats), od, gd, seed=3)
    n = np.abs(PH.normalise(raw, stats))
    assert n.max() == 10.0 and (n < 10.0).any()
    for k in a:
        assert PH.bits(a[k]) == PH.bits(b[k]), k


@pytest.mark.parametrize("A", PH.ACT_DIMS)
def test_noise_against_float64_with_float32_numpy_as_the_yardstick(A):
    """z = (action - mean) / exp(log_std) of a stochastic call against Box-Muller in float64 on the same Philox words.  Bound:
    four times the largest deviation of the float32 NumPy evaluation of the same formulas from float64 on those words.
    Measured: the recovered z deviates by at most 4.4e-7 (the rounding of `action` divided by std is part of it), float32 NumPy
    by 1.2e-6 (its angle 2 pi u is rounded before the cosine), so the bound is 4.9e-6."""
    od, gd = PH.WIDTHS[0]
    c = PH.case(od, gd, A, 1.0)
    calls = np.array([5], np.int64)
    out = PH.host_act(c["w"], c["rows"], od, gd, seed=77, row_offset=123456, calls=calls)
    assert calls[0] == 6
    words = PH.noise_words(77, 123456 + np.arange(PH.ROWS), 5, A)
    z64, z32 = PH.box_muller(words, np.float64)[:, :A], PH.box_muller(words, np.float32)[:, :A]
    std = np.exp(c["w"]["log_std"].astype(np.float64))
    z = (out["action"].astype(np.float64) - c["det"]["action"].astype(np.float64)) / std
    yard, got = float(np.abs(z32 - z64).max()), float(np.abs(z - z64).max())
    print("A %d: recovered z - float64 %.3g; float32 NumPy - float64 %.3g; bound %.3g" % (A, got, yard, 4 * yard))
    assert got <= 4.0 * yard


def _unit_model(A=4):
    """mean 0 and log_std 0: the action IS z"""
    model = PH.make_model(14, A)
    with torch.no_grad():
        model.pi[4].weight.zero_()
        model.pi[4].bias.zero_()
        model.log_std.zero_()
    return PH.weights_of(model)


_noise = {}


def _draws():
    if not _noise:
        w, rows = _unit_model(), np.zeros((65536, 14), np.float32)
        calls = np.array([9], np.int64)
        for k in ("c0", "c1"):
            _noise[k] = PH.host_act(w, rows, 8, 3, seed=2024, calls=calls, logp=False, value=False)["action"]
        _noise["w"] = w
    return _noise


def test_noise_statistics():
    """65 536 rows x 4 columns, two consecutive calls.  Derived 4-sigma bounds: the mean of N standard normals has deviation
    1 / sqrt(N), their variance sqrt(2 / N), a sample correlation of n pairs 1 / sqrt(n); |z| <= sqrt(-2 ln 2^-24) = 5.768."""
    d = _draws()
    z = d["c0"].astype(np.float64)
    N = z.size
    assert N == 262144 and np.isfinite(z).all()
    assert abs(z.mean()) < 4 / np.sqrt(N)
    assert abs(z.var() - 1.0) < 4 * np.sqrt(2.0 / N)
    assert np.abs(z).max() <= 5.77

    def corr(a, b):
        return abs(float(np.corrcoef(a.ravel(), b.ravel())[0, 1])), 4 / np.sqrt(a.size)
    for k in range(3):                                        # adjacent columns (inside a Box-Muller pair and across pairs)
        r, bound = corr(z[:, k], z[:, k + 1])
        assert r < bound, k
    r, bound = corr(z[:-1], z[1:])                           # adjacent rows
    assert r < bound
    r, bound = corr(z, d["c1"].astype(np.float64))           # call c and call c + 1 of the same row
    assert r < bound


def test_noise_differs_with_seed_row_offset_and_calls():
    d = _draws()
    w, rows = d["w"], np.zeros((64, 14), np.float32)
    draw = lambda **kw: PH.host_act(w, rows, 8, 3, logp=False, value=False, **kw)["action"]
    base = draw(seed=2024, calls=np.array([9], np.int64))
    assert PH.bits(base) == PH.bits(d["c0"][:64])
    assert not (d["c0"] == d["c1"]).any()
    for other in (draw(seed=2025, calls=np.array([9], np.int64)), draw(seed=2024, row_offset=64, calls=np.array([9], np.int64)),
                  draw(seed=2024, calls=np.array([10], np.int64)), draw(seed=2024, calls=np.array([9 + (1 << 32)], np.int64))):
        assert not (other == base).any()
    assert PH.bits(draw(seed=2024, row_offset=64, calls=np.array([9], np.int64))) == PH.bits(d["c0"][64:128])   # the global row keys it
    assert PH.bits(draw(seed=2024, calls=np.array([10], np.int64))) == PH.bits(d["c1"][:64])


@pytest.mark.parametrize("A", PH.ACT_DIMS)
@pytest.mark.parametrize("od,gd", PH.WIDTHS[:3])
def test_logp_env_action_and_row_independence(od, gd, A):
    """logp against Normal(mean, std).log_prob(action).sum(-1) under the forward rule (float64 restatement of that expression at
    the call's own action; yardstick: torch's float32 evaluation of it), env_action the exact clamp, and row e of 1000 equal,
    bit for bit, to a batch of one with row_offset = e"""
    c = PH.case(od, gd, A, 1.0)
    calls = np.array([2], np.int64)
    out = PH.host_act(c["w"], c["rows"], od, gd, seed=5, calls=calls)
    a64 = out["action"].astype(np.float64)
    ls = c["w"]["log_std"].astype(np.float64)
    lp64 = (-((a64 - c["mean64"]) ** 2) / (2 * np.exp(ls) ** 2) - ls - 0.5 * np.log(2 * np.pi)).sum(-1)
    with torch.no_grad():
        lp32 = c["model"].dist(torch.from_numpy(c["rows"])).log_prob(torch.from_numpy(out["action"])).sum(-1).numpy()
    yard = float(np.abs(lp32 - lp64).max())
    tol = 2.0 * yard + float(PH.ulp32(np.abs(lp64).max()))
    got = float(np.abs(out["logp"] - lp64).max())
    print("D %d A %d: logp host core - float64 %.3g; torch float32 - float64 %.3g; tolerance %.3g" % (c["D"], A, got, yard, tol))
    assert got <= tol
    assert PH.bits(out["env_action"]) == PH.bits(np.clip(out["action"], -1, 1))
    assert (np.abs(out["action"]) > 1).any() or A == 1
    assert PH.bits(out["value"]) == PH.bits(c["det"]["value"])                  # the value does not see the noise
    for e in (0, 7, 31, 32, 999):
        one = PH.host_act(c["w"], c["rows"][e:e + 1], od, gd, seed=5, row_offset=e, calls=np.array([2], np.int64))
        for k in out:
            assert PH.bits(one[k]) == PH.bits(out[k][e:e + 1]), (e, k)
    # null logp / value: the other outputs do not move
    part = PH.host_act(c["w"], c["rows"][:33], od, gd, seed=5, calls=np.array([2], np.int64), logp=False, value=False)
    assert PH.bits(part["action"]) == PH.bits(out["action"][:33]) and part["logp"] is None and part["value"] is None


def test_elementary_functions_against_float64():
    """tanh, exp, log (on the uniforms) and the sine / cosine of 2 pi m / 2^24 as the core spells them out.  Bound 2 ulp for the
    first three: each ends in a polynomial whose own error is below half an ulp (the Cephes single-precision fits) followed by at
    most three rounded operations of half an ulp each; 2^-22 absolute for sine and cosine (|value| <= 1: an ulp is at most 2^-24,
    the same count, plus half an ulp of the angle's own rounding at |angle| <= pi / 4).  Measured: 1.30, 1.01, 0.82 ulp, 1.1e-7."""
    L = PH.lib()

    def f(fn, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        fn(x.ctypes.data, y.ctypes.data, x.size)
        return x.astype(np.float64), y.astype(np.float64)
    ulps = lambda y, ref: float((np.abs(y - ref) / PH.ulp32(ref)).max())
    rng = np.random.RandomState(0)
    x, y = f(L.ph_tanh, np.concatenate([np.linspace(-12, 12, 200001), rng.uniform(-1, 1, 100000), [0.625, -0.625, 10.0, 50.0]]))
    x2, y2 = f(L.ph_exp, np.linspace(-87, 88, 300001))
    m = np.concatenate([rng.randint(1, 2 ** 24 + 1, 300000), [1, 2, 2 ** 24 - 1, 2 ** 24, 2 ** 22, 3 * 2 ** 21, 2 ** 23]]).astype(np.uint32)
    u, lg = f(L.ph_log, m.astype(np.float64) * 2.0 ** -24)
    nz = u != 1.0
    c, s = np.empty(m.size, np.float32), np.empty(m.size, np.float32)
    L.ph_sincos_turn(m.ctypes.data, c.ctypes.data, s.ctypes.data, m.size)
    th = 2 * np.pi * m.astype(np.float64) * 2.0 ** -24
    got = (ulps(y, np.tanh(x)), ulps(y2, np.exp(x2)), ulps(lg[nz], np.log(u[nz])), float(max(np.abs(c - np.cos(th)).max(), np.abs(s - np.sin(th)).max())))
    print("tanh %.2f ulp, exp %.2f ulp, log %.2f ulp, sine / cosine %.3g absolute" % got)
    assert got[0] <= 2 and got[1] <= 2 and got[2] <= 2 and got[3] <= 2.0 ** -22
    assert lg[~nz].tolist() == [0.0] and np.abs(y).max() == 1.0 and bool((np.abs(y) <= 1).all())


def test_k_order_table_is_the_mfma_accumulator_order():
    k = np.empty(64, np.int32)
    PH.lib().ph_kord(k.ctypes.data)
    expect = [32 * t + 8 * (r >> 2) + 4 * h + (r & 3) for t in range(2) for r in range(16) for h in range(2)]
    assert k.tolist() == expect and sorted(expect) == list(range(64))


def test_device_class_has_no_host_path():
    from gym_xarm_amd.device_policy import DevicePolicy
    from gym_xarm_amd.train import ActorCritic
    p = DevicePolicy(ActorCritic(14, 4))
    with pytest.raises(ValueError, match="ActorCritic"):
        p.act(torch.zeros(3, 14))
    with pytest.raises(ValueError, match="64-64"):
        m = ActorCritic(14, 4)
        m.pi[0] = torch.nn.Linear(14, 32)
        DevicePolicy(m)
    with pytest.raises(ValueError, match="out of range"):
        DevicePolicy(ActorCritic(14, 17))
    import inspect
    from gym_xarm_amd import train
    assert inspect.signature(train.train).parameters["device_policy"].default is False


def test_abi_argument_errors():
    from gym_xarm_amd import _native
    L = _native.load()
    err = lambda: L.xarm_last_error(None).decode()
    lay = lambda E=1000, od=24, gd=3, A=4, hid=64, off=0: C.byref(_native.XarmPolicyLayout(E, od, gd, A, hid, off))
    par = lambda seed=0, clip=10.0, eps=1e-8, det=0: C.byref(_native.XarmPolicyParams(seed, clip, eps, det))
    # any non-null, 16-byte aligned value: every call below with num_envs > 0 fails a check, and the checks come before any launch
    x = 64
    wts = lambda **kw: C.byref(_native.XarmPolicyWeights(*[kw.get(k, x) for k in _native.POLICY_WEIGHT_FIELDS]))
    names = ("stats", "calls", "obs", "ag", "dg", "action", "env_action", "logp", "value")

    def act(l=None, p=None, w=None, **nulls):
        return L.xarm_policy_act(l or lay(), p or par(), w or wts(), *[nulls.get(k, x) for k in names], None)
    for kw, word in ((dict(E=-1), "num_envs"), (dict(od=0), "obs_dim"), (dict(gd=-1), "goal_dim"), (dict(od=95, gd=1), "XARM_POLICY_MAX_DIM"),
                     (dict(od=97, gd=0), "XARM_POLICY_MAX_DIM"), (dict(A=0), "act_dim"), (dict(A=17), "act_dim"), (dict(hid=32), "hidden"),
                     (dict(hid=128), "hidden"), (dict(off=-1), "row_offset")):
        assert act(l=lay(**kw)) == -1 and word in err(), kw
    assert L.xarm_policy_act(None, par(), wts(), *([x] * 9), None) == -1 and "layout" in err()
    assert L.xarm_policy_act(lay(), None, wts(), *([x] * 9), None) == -1 and "params" in err()
    assert L.xarm_policy_act(lay(), par(), None, *([x] * 9), None) == -1 and "weights" in err()
    for kw, word in ((dict(eps=0.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"), (dict(clip=0.0), "clip_obs"),
                     (dict(clip=float("nan")), "clip_obs")):
        assert act(p=par(**kw)) == -1 and word in err(), kw
        assert act(l=lay(E=0), p=par(**kw), stats=None) == 0, kw                  # without stats the two are not read
    # each required pointer, one at a time
    for k in _native.POLICY_WEIGHT_FIELDS:
        assert act(w=wts(**{k: None})) == -1 and "weight pointer" in err(), k
    for k in ("pi_b1", "pi_w2", "pi_b2", "pi_w3", "vf_b1", "vf_w2", "vf_b2", "vf_w3"):
        assert act(w=wts(**{k: 68})) == -1 and "16-byte" in err(), k
    for k in ("calls", "obs", "ag", "dg", "action", "env_action"):
        assert act(**{k: None}) == -1 and "NULL" in err(), k
    # what may be null: no error from the argument checks (a launch follows: not made here)
    empty = lay(E=0)
    assert act(l=empty) == 0
    assert L.xarm_policy_act(empty, par(), wts(), *([None] * 9), None) == 0        # no env: nothing to launch, nothing read
    assert L.xarm_policy_act(lay(E=0, od=97, gd=0), par(), wts(), *([None] * 9), None) == -1
    assert (_native.POLICY_MAX_DIM, _native.POLICY_MAX_ACT, _native.POLICY_HIDDEN) == (96, 16, 64)
    assert C.sizeof(_native.XarmPolicyLayout) == 32 and C.sizeof(_native.XarmPolicyParams) == 32 and C.sizeof(_native.XarmPolicyWeights) == 104
    assert _native.XarmPolicyLayout.row_offset.offset == 24


def _have_sanitizers():
    """libasan / libubsan are installed and a sanitized program starts in this environment"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "san_probe")
        return subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", exe], input=b"int main(){return 0;}",
                              capture_output=True).returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason="libasan/libubsan not available")
def test_host_core_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """every batch size, width and mode through the host core as a stand-alone program (its own main, never loaded into python)"""
    exe = str(tmp_path / "policy_main_san")
    src = os.path.join(PH.DIR, "policy_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "policy_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
