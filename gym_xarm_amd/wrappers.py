"""Observation wrappers on the batched VecEnvs."""
import torch


class PixelObservation:
    """Pixel observations for pixel-based RL: after every reset() and step() of a dict-observation VecEnv, render all E envs
    (xarm_render) and add obs['pixels'] (uint8 [E, H, W, 3], a view of the first 3 channels of the RGBA buffer)
    and, with depth=True, obs['depth'] (float32 [E, H, W], view-axis metres).

    The images go into buffers allocated once here, on the env's current stream, so step() adds no allocation and no host
    sync (a step can be captured into a graph).  The tensors are the wrapper's persistent buffers: the next step overwrites them.

    Terminal frames: with auto-reset an env whose episode ended in this step shows the first frame of its NEW episode (the
    observation rows hold the new episode too); info['terminal_observation'] carries no pixels.  With auto_reset='lazy' the
    env shows its terminal frame in the step that ends the episode, and the reset ticks of the following steps.
    camera: dict of xarm_camera fields overriding the env kind's default camera (VecEnv.default_camera).

    views: instead of the one camera, V views per env in one launch (xarm_render_views) - what VecEnv.render's
    views= takes: names of VecEnv.default_views() ('world', 'wrist0', 'wrist1'), [16] rows, a [V, 16] tensor, or an
    [E, V, 16] tensor with one set per env.  obs['pixels'] is then [E, V, H, W, 3] and obs['depth'] [E, V, H, W].  The records
    live in the device tensor self.views, which the kernel reads at every step: write into it in place (self.views.copy_(...))
    to move the cameras, also between the replays of a captured step."""

    def __init__(self, venv, width=84, height=84, camera=None, depth=False, views=None):
        self.venv = venv
        self.num_envs = venv.num_envs
        dev, E = venv.device, venv.num_envs
        self.views = None
        if views is not None:
            if camera is not None:
                raise ValueError("camera= and views= exclude each other")
            self.views, self._per_env = venv._views(views, E)
            H, W, shape = int(height), int(width), (E, self.views.shape[-2], int(height), int(width))
        else:
            self._cam = venv._camera(camera, width, height)
            H, W = self._cam.height, self._cam.width
            shape = (E, H, W)
        self._size = (W, H)
        self._rgba = torch.zeros(*shape, 4, device=dev, dtype=torch.uint8)
        self._depth = torch.zeros(*shape, device=dev, dtype=torch.float32) if depth else None
        self.pixels = self._rgba[..., :3]

    def _add(self, obs):
        if not isinstance(obs, dict):
            raise TypeError("PixelObservation wraps a dict-observation VecEnv (got %s)" % type(obs).__name__)
        if self.views is not None:
            self.venv.render_views_into(self.views, self._per_env, self._size[0], self._size[1], 0, None, self._rgba, self._depth)
        else:
            self.venv.render_into(self._cam, None, self._rgba, self._depth)
        obs = dict(obs)
        obs["pixels"] = self.pixels
        if self._depth is not None:
            obs["depth"] = self._depth
        return obs

    def reset(self, mask=None):
        return self._add(self.venv.reset(mask))

    def step(self, actions):
        obs, rew, done, info = self.venv.step(actions)
        return self._add(obs), rew, done, info

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, info = self.venv.step_wait()
        return self._add(obs), rew, done, info

    def __getattr__(self, name):
        return getattr(self.venv, name)
