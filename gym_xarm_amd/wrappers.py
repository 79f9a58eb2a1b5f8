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
    camera: dict of xarm_camera fields overriding the env kind's default camera (VecEnv.default_camera)."""

    def __init__(self, venv, width=84, height=84, camera=None, depth=False):
        self.venv = venv
        self.num_envs = venv.num_envs
        self._cam = venv._camera(camera, width, height)
        dev, E, H, W = venv.device, venv.num_envs, self._cam.height, self._cam.width
        self._rgba = torch.zeros(E, H, W, 4, device=dev, dtype=torch.uint8)
        self._depth = torch.zeros(E, H, W, device=dev, dtype=torch.float32) if depth else None
        self.pixels = self._rgba[..., :3]

    def _add(self, obs):
        if not isinstance(obs, dict):
            raise TypeError("PixelObservation wraps a dict-observation VecEnv (got %s)" % type(obs).__name__)
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
