"""View records on the MI355X: k_render_views (csrc/xarm_k_render.hip) against the host build of the same core and the NumPy
checker, its call contract (V views per call, shared / per-env records, subsets, invalid records and arguments), that it never
changes the simulation, that a captured call follows in-place changes of the views, and the Python surface on top of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_ref as R
import render_views_host as VH
import render_views_ref as VR
from test_render_gpu import KIND_IDS, _env_of, _np
from test_render_host import states
from test_render_views_host import invalid_records

pytestmark = pytest.mark.gpu
W, H = 48, 40
KEYS = ("rgba", "depth", "seg")


@pytest.fixture(scope="module")
def gx():
    import gym_xarm_amd
    return gym_xarm_amd


def _views_of(env):
    return torch.stack(list(env.default_views().values()))


def _device_vs_host(kind, out, host):
    """the device rule of tests/test_render_gpu.py: seg >= 99.9 %, RGB <= 2 levels, depth 1e-4 m off the boundary band, 1e-3 m on it"""
    h_rgba, h_depth, h_seg = host
    rgba, depth, seg = _np(out["rgba"]), _np(out["depth"]), _np(out["seg"])
    agree = seg == h_seg
    dd = np.abs(depth - h_depth)
    bnd = np.stack([R.boundary(x) for x in h_seg.reshape(-1, *h_seg.shape[2:])]).reshape(h_seg.shape)
    dc = np.abs(rgba.astype(int) - h_rgba.astype(int)).max(-1)
    print(kind, "seg agree %.5f" % agree.mean(), "depth off band %.2e on band %.2e" % (dd[agree & ~bnd].max(), dd[agree].max()),
          "rgb", dc[agree].max())
    assert agree.mean() >= 0.999, (kind, agree.mean())
    assert dd[agree & ~bnd].max() <= 1e-4 and dd[agree].max() <= 1e-3, (kind, dd[agree & ~bnd].max(), dd[agree].max())
    assert dc[agree].max() <= 2, kind
    return rgba, depth, seg


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_device_matches_the_host_core_and_the_checker(gx):
    for kind, rows, nobj in states():
        env = _env_of(gx, kind, rows, nobj)
        views = _views_of(env)
        assert views.shape == (1 + VR.NARMS[kind], 16)
        for w, h in ((W, H), (64, 64)):
            out = env.render(width=w, height=h, env_ids=list(range(len(rows))), views=views, depth=True, segmentation=True)
            torch.cuda.synchronize()
            st = _np(env.get_state())
            rgba, depth, seg = _device_vs_host(kind, out, VH.render(kind, st, _np(views), w, h, num_obj=nobj))
            VR.assert_matches_checker(kind, st.astype(np.float64), _np(views), rgba, depth, seg, num_obj=nobj)
        env.close()


def test_rearrange_device_matches_the_host_core(gx):
    env = gx.make("XarmRearrange-v0", num_envs=3, seed=1)
    env.reset()
    env.step(torch.rand(3, 8, device="cuda") * 2 - 1)
    views = _views_of(env)
    assert views.shape == (3, 16)
    out = env.render(width=W, height=H, env_ids=[0, 1, 2], views=views, depth=True, segmentation=True)
    torch.cuda.synchronize()
    _, _, seg = _device_vs_host("rearrange", out, VH.render("rearrange", _np(env.get_state()), _np(views), W, H))
    assert (seg[:, 1] == 3).any() and (seg[:, 2] == 5).any() and (seg[:, 0] == 11).any()   # both grippers, the fourth cube
    env.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_view_batching_subsets_and_permutations_are_bit_exact(gx):
    E = 64
    env = gx.make("XarmPDHandover-v0", num_envs=E, seed=5)
    env.reset()
    env.step(torch.rand(E, 8, device="cuda") * 2 - 1)
    views = _views_of(env)                                                         # V = 3
    kw = dict(width=W, height=H, depth=True, segmentation=True)
    full = env.render(env_ids=list(range(E)), views=views, **kw)
    assert full["rgba"].shape == (E, 3, H, W, 4) and full["depth"].shape == (E, 3, H, W) and full["seg"].shape == (E, 3, H, W)
    for v in range(3):                                                             # a V = 3 call = three V = 1 calls
        one = env.render(env_ids=list(range(E)), views=views[v:v + 1], **kw)
        for k in KEYS:
            assert torch.equal(one[k][:, 0], full[k][:, v]), (k, v)
    per = views[None].repeat(E, 1, 1)                                              # per_env with identical rows = shared
    per_out = env.render(env_ids=list(range(E)), views=per, **kw)
    for k in KEYS:
        assert torch.equal(per_out[k], full[k]), k
    ids = [37, 3, 63, 0, 12, 5]
    jit = per + 0.01 * torch.randn(E, 3, 16, device="cuda") * (torch.arange(16, device="cuda") < 9)   # eye / target / up differ per env
    full_j = env.render(env_ids=list(range(E)), views=jit, **kw)
    assert not torch.equal(full_j["rgba"], full["rgba"])
    for vs, ref in ((views, full), (jit[ids], full_j)):                            # subsets and permutations, with views[ids]
        part = env.render(env_ids=ids, views=vs, **kw)
        for k in KEYS:
            assert torch.equal(part[k], ref[k][ids]), k
    env.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_per_env_views_differ_and_equal_single_env_renders(gx):
    E = 16
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=9, auto_reset=False)
    env.reset()
    env.set_state(env.get_state()[3:4].repeat(E, 1))                               # one state, E times
    base = env.default_views()["world"]
    views = base[None, None].repeat(E, 1, 1)
    views[:, 0, 0:3] += 0.3 * (torch.rand(E, 3, device="cuda") - 0.5)              # 16 jittered eyes
    out = env.render(width=W, height=H, env_ids=list(range(E)), views=views, depth=True, segmentation=True)
    for e in range(E):
        one = env.render(width=W, height=H, env_ids=[e], views=views[e], depth=True, segmentation=True)
        for k in KEYS:
            assert torch.equal(one[k][0], out[k][e]), (k, e)
    assert len({_np(out["rgba"][e]).tobytes() for e in range(E)}) >= 2
    env.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,narms", [("XarmPDPickAndPlace-v0", 1), ("XarmPDStackTower-v0", 2)])
def test_invalid_records_give_the_invalid_image_for_exactly_those_views(gx, env_id, narms):
    good, bad = invalid_records(narms)
    E, V = len(bad) + 4, 2
    env = gx.make(env_id, num_envs=E, seed=2)
    env.reset()
    views = torch.stack([torch.as_tensor(good).cuda(), env.default_views()["wrist0"]])[None].repeat(E, 1, 1)
    kw = dict(width=W, height=H, env_ids=list(range(E)), depth=True, segmentation=True)
    ref = env.render(views=views, **kw)
    where = {}
    for i, (why, rec) in enumerate(bad.items()):                                   # in the middle of the batch, alternating views
        where[(2 + i, i % V)] = why
        views[2 + i, i % V] = torch.as_tensor(rec)
    scratch = torch.empty_like(ref["rgba"])
    rc = env._L.xarm_render_views(env._h, C.c_void_p(views.data_ptr()), V, 1, W, H, 0, None, E, C.c_void_p(scratch.data_ptr()), None, None,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0                                                                 # the call itself succeeds
    out = env.render(views=views, **kw)
    torch.cuda.synchronize()                                                       # raises if a HIP error is pending
    assert torch.ones(1, device="cuda").item() == 1.0
    assert torch.equal(scratch, out["rgba"])
    for e in range(E):
        for v in range(V):
            if (e, v) in where:
                assert (out["rgba"][e, v] == 0).all() and (out["depth"][e, v] == 0).all() and (out["seg"][e, v] == 255).all(), where[(e, v)]
            else:
                for k in KEYS:
                    assert torch.equal(out[k][e, v], ref[k][e, v]), (k, e, v)
    assert (ref["seg"] != 255).all()
    env.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_with_a_message(gx):
    from gym_xarm_amd import _native
    env = gx.make("XarmReach-v0", num_envs=8, seed=0)
    env.reset()
    L, h = env._L, env._h
    views = _views_of(env)                                                         # world, wrist0
    rgba = torch.zeros(8, 2, 16, 16, 4, device="cuda", dtype=torch.uint8)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp, rp = C.c_void_p(views.data_ptr()), C.c_void_p(rgba.data_ptr())

    def call(views=vp, V=2, per_env=0, w=16, hh=16, flags=0, n=8, out=rp):
        return L.xarm_render_views(h, views, V, per_env, w, hh, flags, None, n, out, None, None, st)
    assert call() == 0
    M = _native.RENDER_MAX_DIM
    for kw in (dict(views=None), dict(out=None), dict(V=0), dict(V=_native.RENDER_MAX_VIEWS + 1), dict(w=0), dict(hh=-1), dict(w=M + 1),
               dict(hh=M + 1), dict(n=0), dict(n=9), dict(flags=8), dict(per_env=2)):
        assert call(**kw) == -1, kw
        assert b"xarm_render_views" in L.xarm_last_error(h), kw
    v = (C.c_float * 16)()
    assert L.xarm_default_view(h, 2, v) == -1 and b"xarm_default_view" in L.xarm_last_error(h)   # a one-arm kind
    assert L.xarm_default_view(h, 3, v) == -1 and L.xarm_default_view(h, 1, v) == 0 and v[12] == 1.0
    assert list(env.default_views()) == ["world", "wrist0"]
    with pytest.raises(ValueError):
        env.render(views=["world"], camera={"fov_deg": 50.0})
    with pytest.raises(ValueError):
        env.render(views=["wrist1"])
    with pytest.raises(ValueError):
        env.render(views=torch.zeros(3, 2, 16), env_ids=[0, 1])                    # [n, V, 16] with the wrong n
    with pytest.raises(_native.XarmNativeError):
        env.render(views=["world"] * (_native.RENDER_MAX_VIEWS + 1), width=8, height=8)
    torch.cuda.synchronize()
    env.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,A", [("XarmPDPickAndPlace-v0", 4), ("XarmPDHandover-v0", 8)])
def test_rendering_views_never_changes_the_simulation(gx, env_id, A):
    E = 4096

    def run(render):
        env = gx.make(env_id, num_envs=E, seed=7)
        env.reset()
        gen = torch.Generator(device="cuda").manual_seed(1)
        rec = []
        for _ in range(20):
            obs, rew, done, info = env.step(torch.rand(E, A, device="cuda", generator=gen) * 2 - 1)
            if render:
                env.render(width=32, height=32, env_ids=list(range(0, E, 7)), views=["wrist0", "world"], depth=True, segmentation=True)
            rec.append(torch.cat([obs["observation"], rew[:, None], done[:, None].float(), env.get_state()], 1).clone())
        torch.cuda.synchronize()
        env.close()
        return torch.stack(rec)
    assert torch.equal(run(False), run(True))


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_captured_step_and_render_views_follow_the_views_tensor(gx):
    E, A, V = 512, 4, 2
    gen = torch.Generator(device="cuda").manual_seed(0)
    acts = [torch.rand(E, A, device="cuda", generator=gen) * 2 - 1 for _ in range(5)]

    def run(capture):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=2)
        env.reset()
        dv = env.default_views()
        first = torch.stack([dv["world"], dv["wrist0"]])
        second = first.clone()
        second[0, 0:3] += torch.tensor([0.2, -0.1, 0.3], device="cuda")            # another world eye
        second[1, 9] = 50.0                                                        # a narrower wrist camera
        views = first.clone()
        rgba = torch.zeros(E, V, 24, 32, 4, device="cuda", dtype=torch.uint8)
        seg = torch.zeros(E, V, 24, 32, device="cuda", dtype=torch.uint8)
        a = acts[0].clone()

        def both():
            env.step(a)
            env.render_views_into(views, 0, 32, 24, 0, None, rgba, None, seg)
        outs = []
        if capture:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                both()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                both()
        else:
            both()
        for k in range(1, 5):
            a.copy_(acts[k])
            views.copy_(second if k >= 3 else first)                               # in place, between replays
            g.replay() if capture else both()
            outs.append((rgba.clone(), seg.clone()))
        torch.cuda.synchronize()
        env.close()
        return outs
    eager, graph = run(False), run(True)
    for (r0, s0), (r1, s1) in zip(eager, graph):
        assert torch.equal(r0, r1) and torch.equal(s0, s1)
    assert not torch.equal(eager[1][1], eager[2][1])                               # the new views show in the images


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_pixel_observation_with_views(gx):
    from gym_xarm_amd.wrappers import PixelObservation
    E, cam = 64, {"yaw_deg": 60.0, "distance": 1.0}
    venv = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=3)
    env = PixelObservation(venv, width=W, height=H, views=[venv.view_from_camera(cam), "wrist0"], depth=True)
    old = PixelObservation(venv, width=W, height=H, camera=cam, depth=True)
    env.reset()
    obs, rew, done, info = env.step(torch.zeros(E, 4, device="cuda"))
    assert obs["pixels"].shape == (E, 2, H, W, 3) and obs["depth"].shape == (E, 2, H, W) and env.views.shape == (2, 16)
    want = old._add({})                                                            # the old wrapper's pixels of the same states
    assert want["pixels"].shape == (E, H, W, 3)
    seg = venv.render(width=W, height=H, env_ids=list(range(E)), camera=cam, segmentation=True)["seg"]
    torch.cuda.synchronize()
    # the rule of item 1 (the basis is built in float32 in the kernel, in double on the host: not bitwise)
    bnd = np.stack([R.boundary(x) for x in _np(seg)])
    dc = np.abs(_np(obs["pixels"][:, 0]).astype(int) - _np(want["pixels"]).astype(int)).max(-1)
    dd = np.abs(_np(obs["depth"][:, 0]) - _np(want["depth"]))
    same = dc <= 2
    print("pixels within 2 levels %.5f" % same.mean(), "depth off band %.2e" % dd[same & ~bnd].max(), "on band %.2e" % dd[same].max())
    assert same.mean() >= 0.999 and not (~same & ~bnd).any()
    assert dd[same & ~bnd].max() <= 1e-4 and dd[same].max() <= 1e-3
    assert not torch.equal(obs["pixels"][:, 0], obs["pixels"][:, 1])
    plain = PixelObservation(venv, width=W, height=H)                              # without views: as before
    assert plain.reset()["pixels"].shape == (E, H, W, 3)
    venv.close()


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_single_env_render_takes_a_view(gx):
    for env_id in gx.registered_ids():
        one = gx.make(env_id)
        one.reset()
        img = one.render(view="wrist0", width=40, height=30)
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (30, 40, 4) and (img[..., 3] == 255).all(), env_id
        assert not np.array_equal(img, one.render(view="world", width=40, height=30)), env_id
        vec = one._vec if hasattr(one, "_vec") else one._env._vec                 # the NoGoal id wraps the single-env class
        two = len(vec.default_views()) == 3
        if two:
            assert one.render(view="wrist1", width=40, height=30).shape == (30, 40, 4)
        else:
            with pytest.raises(ValueError):
                one.render(view="wrist1")
        one.close()
