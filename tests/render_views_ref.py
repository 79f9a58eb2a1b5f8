"""Independent float64 NumPy checker of the view records (include/xarm_hip.h "views", csrc/xarm_render_core.h rc_make_view):
a look-at camera in a mount frame, and the validity rule stated on its own.  The hand frames come from the oracle's FK through
render_ref.arm_frames; nothing here reads the render core.  ViewCamera is what render_ref.render takes as its camera."""
import numpy as np

import render_ref as R

MOUNT_WORLD, MOUNT_HAND0, MOUNT_HAND1 = 0, 1, 2
NARMS = {k: R.LAYOUT[k]["narms"] for k in R.KINDS}


def record(mount, eye, target, up, fov, near, far):
    v = np.zeros(16, dtype=np.float32)
    v[0:3], v[3:6], v[6:9], v[9], v[10], v[11], v[12] = eye, target, up, fov, near, far, mount
    return v


def valid(view, narms):
    """the validity rule: floats 0-12 finite; mount exactly 0, 1 or 2 and a hand mount names an arm the scene has;
    0 < fov < 180; 0 < near < far < 1e30; |target - eye| > 1e-6; |up| > 1e-6; |f x up / |up|| > 1e-6"""
    v = np.asarray(view, dtype=np.float64)
    if not np.isfinite(v[:13]).all():
        return False
    if v[12] not in (0.0, 1.0, 2.0) or v[12] > narms:
        return False
    if not (0 < v[9] < 180 and 0 < v[10] < v[11] < 1e30):
        return False
    d, up = v[3:6] - v[0:3], v[6:9]
    if not (np.linalg.norm(d) > 1e-6 and np.linalg.norm(up) > 1e-6):
        return False
    return bool(np.linalg.norm(np.cross(d / np.linalg.norm(d), up / np.linalg.norm(up))) > 1e-6)


def mount_frame(kind, row, mount):
    """(R, p) of the mount in the world: the identity, or the hand frame of arm mount - 1 in the state row"""
    if mount == MOUNT_WORLD:
        return np.eye(3), np.zeros(3)
    arm = mount - 1
    q0 = R.LAYOUT[kind]["q"] + 9 * arm
    q = np.asarray(row[q0:q0 + (13 if kind == "reach" else 9)], dtype=np.float64)
    return R.arm_frames(kind, q, arm)[1]


class ViewCamera:
    """the camera of a valid view record for one env: eye, f / s / u (unit), tx / ty, rays() - render_ref.Camera's interface"""

    def __init__(self, view, kind, row, width, height, shadows=False):
        v = np.asarray(view, dtype=np.float64)
        assert valid(v, NARMS[kind])
        Rm, pm = mount_frame(kind, row, int(v[12]))
        self.eye = pm + Rm @ v[0:3]
        self.target = pm + Rm @ v[3:6]
        up = Rm @ v[6:9]
        f = self.target - self.eye
        self.f = f / np.linalg.norm(f)
        s = np.cross(self.f, up)
        self.s = s / np.linalg.norm(s)
        self.u = np.cross(self.s, self.f)
        self.ty = np.tan(np.radians(v[9]) / 2)
        self.tx = self.ty * width / height
        self.width, self.height, self.near, self.far, self.shadows = int(width), int(height), float(v[10]), float(v[11]), shadows

    def rays(self):
        j = np.arange(self.width) + 0.5
        i = np.arange(self.height) + 0.5
        Y, X = np.meshgrid(1 - 2 * i / self.height, 2 * j / self.width - 1, indexing="ij")
        return (self.f[None, None] + self.s[None, None] * (self.tx * X)[..., None] + self.u[None, None] * (self.ty * Y)[..., None]).reshape(-1, 3)


def assert_matches_checker(kind, rows, views, rgba, depth, seg, num_obj=1, seg_frac=0.995):
    """test_render_host.assert_matches_checker's rule for [n, V, H, W] images of shared views [V, 16]"""
    H, W = seg.shape[2:]
    for e in range(len(rows)):
        for v in range(len(views)):
            cam = ViewCamera(views[v], kind, rows[e], W, H)
            r_rgba, r_depth, r_seg = R.render(kind, rows[e], cam, num_obj=num_obj)
            agree = seg[e, v] == r_seg
            bnd = R.boundary(r_seg)
            assert agree.mean() >= seg_frac, (kind, e, v, agree.mean())
            assert not (~agree & ~bnd).any(), (kind, e, v, np.argwhere(~agree & ~bnd)[:5])
            dd = np.abs(depth[e, v].astype(np.float64) - r_depth)
            assert (dd[agree & ~bnd] <= 1e-4).all() and (dd[agree] <= 1e-3).all(), (kind, e, v, dd[agree].max())
            dc = np.abs(rgba[e, v].astype(int) - r_rgba.astype(int)).max(-1)
            assert (dc[agree] <= 2).all(), (kind, e, v, dc[agree].max())
            assert (rgba[e, v][..., 3] == 255).all()
