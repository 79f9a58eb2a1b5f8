"""Rendering on the MI355X: k_render (csrc/xarm_k_render.hip) against the host build of the same core and the NumPy checker,
its call contract (shapes, subsets, invalid arguments), that it never changes the simulation, and that it captures into a graph."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import render_host as RH
import render_ref as R
from test_render_host import assert_matches_checker, states

pytestmark = pytest.mark.gpu
KIND_IDS = {"pick_and_place": "XarmPDPickAndPlace-v0", "reach": "XarmReach-v0", "handover": "XarmPDHandover-v0",
            "stack_tower": "XarmPDStackTower-v0"}


@pytest.fixture(scope="module")
def gx():
    import gym_xarm_amd
    return gym_xarm_amd


def _env_of(gx, kind, rows, num_obj=1, use_stand=False):
    cfg = {"num_obj": num_obj, "use_stand": use_stand} if kind == "handover" else None
    env = gx.make(KIND_IDS[kind], num_envs=len(rows), seed=0, config=cfg, auto_reset=False)
    env.reset()
    env.set_state(torch.as_tensor(np.asarray(rows, dtype=np.float32), device=env.device))
    return env


def _np(x):
    return x.detach().cpu().numpy()


def test_every_registered_id_renders_the_documented_shapes(gx):
    for env_id in gx.registered_ids():
        one = gx.make(env_id)
        one.reset()
        img = one.render()
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4, env_id
        assert (img[..., 3] == 255).all()
        small = one.render(width=40, height=30)
        assert small.shape == (30, 40, 4)
        one.close()
        venv = gx.make(env_id, num_envs=3)
        venv.reset()
        x = venv.render()
        assert x.shape[0] == 1 and x.dtype == torch.uint8 and x.device.type == "cuda" and x.shape[3] == 4
        out = venv.render(width=24, height=16, env_ids=[2, 0], depth=True, segmentation=True)
        assert out["rgba"].shape == (2, 16, 24, 4) and out["depth"].shape == (2, 16, 24) and out["seg"].shape == (2, 16, 24)
        assert out["depth"].dtype == torch.float32 and out["seg"].dtype == torch.uint8
        venv.close()


def test_device_matches_the_host_core_and_the_checker(gx):
    for kind, rows, nobj in states():
        env = _env_of(gx, kind, rows, nobj)
        for W, H in ((64, 64), (128, 96)):
            cam = RH.camera(kind, width=W, height=H)
            h_rgba, h_depth, h_seg = RH.render(kind, _np(env.get_state()), cam, num_obj=nobj)
            out = env.render(width=W, height=H, env_ids=list(range(len(rows))), depth=True, segmentation=True)
            torch.cuda.synchronize()
            rgba, depth, seg = _np(out["rgba"]), _np(out["depth"]), _np(out["seg"])
            agree = seg == h_seg
            assert agree.mean() >= 0.999, (kind, agree.mean())
            # float32 on both sides, rounded differently: the device FK runs on the hardware v_sin_f32 / v_cos_f32 (the physics
            # cores' xsincos, abs. error ~1e-6) and hipcc contracts the ray arithmetic into FMAs; rays grazing a surface (the
            # far ground, silhouettes) turn that into up to ~2e-4 m of depth (measured: 1.8 % of the pixels differ by more than 1e-5 m);
            # the bound is the checker rule's: 1e-4 m off the segmentation boundary band, 1e-3 m on it
            dd = np.abs(depth - h_depth)
            bnd = np.stack([R.boundary(x) for x in h_seg])
            assert dd[agree & ~bnd].max() <= 1e-4 and dd[agree].max() <= 1e-3, (kind, dd[agree & ~bnd].max(), dd[agree].max())
            assert np.mean(dd[agree] > 1e-5) < 0.05, (kind, np.mean(dd[agree] > 1e-5))
            assert np.abs(rgba.astype(int) - h_rgba.astype(int)).max(-1)[agree].max() <= 2, kind
            assert_matches_checker(kind, _np(env.get_state()).astype(np.float64), rgba, depth, seg, cam, num_obj=nobj)
        env.close()


def test_subsets_and_permutations_equal_the_full_batch(gx):
    env = gx.make("XarmPDHandover-v0", num_envs=64, seed=5)
    env.reset()
    env.step(torch.rand(64, 8, device="cuda") * 2 - 1)
    full = env.render(width=48, height=40, env_ids=list(range(64)), depth=True, segmentation=True)
    ids = [37, 3, 63, 0, 12, 5]
    part = env.render(width=48, height=40, env_ids=ids, depth=True, segmentation=True)
    for k in ("rgba", "depth", "seg"):
        assert torch.equal(part[k], full[k][ids]), k
    env.close()


@pytest.mark.parametrize("env_id,A", [("XarmPDPickAndPlace-v0", 4), ("XarmPDHandover-v0", 8)])
def test_rendering_never_changes_the_simulation(gx, env_id, A):
    E = 4096

    def run(render):
        env = gx.make(env_id, num_envs=E, seed=7)
        env.reset()
        gen = torch.Generator(device="cuda").manual_seed(1)
        rec = []
        for _ in range(20):
            obs, rew, done, info = env.step(torch.rand(E, A, device="cuda", generator=gen) * 2 - 1)
            if render:
                env.render(width=32, height=32, env_ids=list(range(0, E, 7)), depth=True, segmentation=True)
            rec.append(torch.cat([obs["observation"], rew[:, None], done[:, None].float(), env.get_state()], 1).clone())
        torch.cuda.synchronize()
        env.close()
        return torch.stack(rec)
    assert torch.equal(run(False), run(True))


def test_captured_step_and_render_replay_like_eager(gx):
    E, A = 512, 4

    def run(capture):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=2)
        env.reset()
        cam = env._camera(None, 32, 24)
        rgba = torch.zeros(E, 24, 32, 4, device="cuda", dtype=torch.uint8)
        seg = torch.zeros(E, 24, 32, device="cuda", dtype=torch.uint8)
        gen = torch.Generator(device="cuda").manual_seed(0)
        acts = [torch.rand(E, A, device="cuda", generator=gen) * 2 - 1 for _ in range(5)]
        a = acts[0].clone()
        outs = []
        if capture:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                env.step(a)
                env.render_into(cam, None, rgba, None, seg)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                env.step(a)
                env.render_into(cam, None, rgba, None, seg)
            for k in range(1, 5):
                a.copy_(acts[k])
                g.replay()
                outs.append((rgba.clone(), seg.clone()))
        else:
            env.step(a)
            env.render_into(cam, None, rgba, None, seg)
            for k in range(1, 5):
                env.step(acts[k])
                env.render_into(cam, None, rgba, None, seg)
                outs.append((rgba.clone(), seg.clone()))
        torch.cuda.synchronize()
        env.close()
        return outs
    for (r0, s0), (r1, s1) in zip(run(False), run(True)):
        assert torch.equal(r0, r1) and torch.equal(s0, s1)


def test_full_size_batch(gx):
    E = 65536
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=4)
    env.reset()
    out = env.render(width=64, height=64, env_ids=torch.arange(E), depth=True, segmentation=True)
    torch.cuda.synchronize()
    seg = out["seg"]
    assert ((seg == 1).flatten(1).any(1)).all() and (((seg == 2) | (seg == 3)).flatten(1).any(1)).all()
    assert not torch.isnan(out["depth"]).any()
    env.close()


def test_invalid_arguments_are_refused_and_bad_ids_give_zero_images(gx):
    from gym_xarm_amd import _native
    env = gx.make("XarmReach-v0", num_envs=8, seed=0)
    env.reset()
    L, h = env._L, env._h
    rgba = torch.zeros(8, 16, 16, 4, device="cuda", dtype=torch.uint8)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = env._camera(None, 16, 16)
    assert L.xarm_render(h, C.byref(good), None, 8, C.c_void_p(rgba.data_ptr()), None, None, st) == 0

    def cam(**kw):
        c = env._camera(None, 16, 16)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for bad in (cam(width=0), cam(height=-1), cam(width=_native.RENDER_MAX_DIM + 1), cam(fov_deg=0.0), cam(fov_deg=180.0),
                cam(near_z=0.0), cam(far_z=0.05), cam(distance=0.0), cam(flags=8)):
        assert L.xarm_render(h, C.byref(bad), None, 8, C.c_void_p(rgba.data_ptr()), None, None, st) == -1
        assert L.xarm_last_error(h)
    assert L.xarm_render(h, C.byref(good), None, 0, C.c_void_p(rgba.data_ptr()), None, None, st) == -1
    assert L.xarm_render(h, C.byref(good), None, 9, C.c_void_p(rgba.data_ptr()), None, None, st) == -1
    assert L.xarm_render(h, C.byref(good), None, 8, None, None, None, st) == -1
    assert L.xarm_render(h, None, None, 8, C.c_void_p(rgba.data_ptr()), None, None, st) == -1
    with pytest.raises(_native.XarmNativeError):
        env.render(width=16, height=16, camera={"fov_deg": 200.0})
    out = env.render(width=16, height=16, env_ids=[3, -1, 8, 1 << 30], depth=True, segmentation=True)
    torch.cuda.synchronize()
    assert (out["rgba"][1:] == 0).all() and (out["depth"][1:] == 0).all() and (out["seg"][1:] == 255).all()
    assert (out["rgba"][0, ..., 3] == 255).all()
    env.close()


def test_pixel_observation_wrapper(gx):
    from gym_xarm_amd.wrappers import PixelObservation
    E = 256
    env = PixelObservation(gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=3), width=40, height=32, depth=True)
    obs = env.reset()
    assert obs["pixels"].shape == (E, 32, 40, 3) and obs["depth"].shape == (E, 32, 40)
    a = torch.zeros(E, 4, device="cuda")
    obs, rew, done, info = env.step(a)
    ref = env.venv.render(width=40, height=32, env_ids=list(range(E)))
    assert torch.equal(obs["pixels"], ref[..., :3])
    # no host sync in step: the wrapped step captures into a graph and replays
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(a)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        obs, rew, done, info = env.step(a)
    g.replay()
    torch.cuda.synchronize()
    ref = env.venv.render(width=40, height=32, env_ids=list(range(E)))
    assert torch.equal(obs["pixels"], ref[..., :3])
    env.close()


def test_sb3_adapter_frames(gx):
    from gym_xarm_amd.sb3_adapter import SB3VecEnv
    v = SB3VecEnv(gx.make("XarmPDPickAndPlace-v0", num_envs=20, seed=0))
    v.reset()
    f = v.render("rgb_array")
    assert f.shape == (500, 500, 3) and f.dtype == np.uint8
    imgs = v.get_images()
    assert len(imgs) == 16 and imgs[0].shape == (500, 500, 3) and np.array_equal(imgs[0], f)
    v.close()
