"""Minimal camera and pose holders for the pose / depth evaluation (eval_utils, eval_pose_pairs).

Same data layout and attribute names as the reference's wrappers (gluefactory/geometry/wrappers.py), so that either kind
of object can be handed to the evaluation functions, which only read `_data` and `model`:

  Camera._data [..., 6 | 8 | 10] = w, h, fx, fy, cx, cy [, k1, k2 [, p1, p2]];  `model` one of CAMERA_MODELS
        (OPENCV_FISHEYE: the four coefficients are k1..k4 of the Kannala-Brandt model).  Pixel centres at +0.5.
  Pose._data   [..., 12] = R row-major, then t  (x_dst = R x_src + t).

Holders only: the projection arithmetic lives in csrc/eval_pose.hip.  `camera_args` / `pose_args` turn holders (or the
reference's wrappers, or plain tensors) into the flat fp32 arrays of the C ABI.
"""
import numpy as np
import torch

from ._native import GFC_CAM_OPENCV, GFC_CAM_OPENCV_FISHEYE, GFC_CAM_PINHOLE, GFC_CAM_RADIAL

CAMERA_MODELS = ("PINHOLE", "RADIAL", "OPENCV", "OPENCV_FISHEYE")
_WIDTH_MODEL = {6: "PINHOLE", 8: "RADIAL", 10: "OPENCV"}


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


class _Holder:
    def __init__(self, data):
        self._data = _tensor(data)

    def _like(self, data):
        new = self.__class__(data)
        if hasattr(self, "model"):
            new.model = self.model
        return new

    shape = property(lambda self: self._data.shape[:-1])
    device = property(lambda self: self._data.device)
    dtype = property(lambda self: self._data.dtype)

    def __getitem__(self, index):
        return self._like(self._data[index])

    def to(self, *args, **kwargs):
        return self._like(self._data.to(*args, **kwargs))

    def cpu(self):
        return self._like(self._data.cpu())

    def cuda(self):
        return self._like(self._data.cuda())

    def float(self):
        return self._like(self._data.float())

    def double(self):
        return self._like(self._data.double())

    @classmethod
    def stack(cls, objects, dim=0):
        new = objects[0]._like(torch.stack([o._data for o in objects], dim=dim))
        if any(getattr(o, "model", None) != getattr(new, "model", None) for o in objects):
            raise ValueError("stacked cameras share one model")
        return new

    def __repr__(self):
        return f"{self.__class__.__name__}: {tuple(self.shape)} {self.dtype} {self.device}"


class Pose(_Holder):
    def __init__(self, data):
        super().__init__(data)
        assert self._data.shape[-1] == 12

    @classmethod
    def from_Rt(cls, R, t):
        R, t = _tensor(R), _tensor(t)
        assert R.shape[-2:] == (3, 3) and t.shape[-1] == 3 and R.shape[:-2] == t.shape[:-1]
        return cls(torch.cat([R.flatten(start_dim=-2), t.to(R.dtype)], -1))

    @classmethod
    def from_4x4mat(cls, T):
        T = _tensor(T)
        assert T.shape[-2:] == (4, 4)
        return cls.from_Rt(T[..., :3, :3], T[..., :3, 3])

    @property
    def R(self):
        return self._data[..., :9].reshape(self._data.shape[:-1] + (3, 3))

    @property
    def t(self):
        return self._data[..., 9:]

    def inv(self):
        Rt = self.R.transpose(-1, -2)
        return self.__class__.from_Rt(Rt, -(Rt @ self.t.unsqueeze(-1)).squeeze(-1))

    def compose(self, other):
        """self @ other: the pose that applies `other` first (T_A2C = T_B2C @ T_A2B)."""
        return self.__class__.from_Rt(self.R @ other.R, self.t + (self.R @ other.t.unsqueeze(-1)).squeeze(-1))

    __matmul__ = compose


class Camera(_Holder):
    def __init__(self, data, model=None):
        super().__init__(data)
        width = self._data.shape[-1]
        assert width in _WIDTH_MODEL, f"camera data of width {width}: 6, 8 or 10 expected"
        self.model = model or _WIDTH_MODEL[width]

    @classmethod
    def from_calibration_matrix(cls, K):
        K = _tensor(K)
        cx, cy, fx, fy = K[..., 0, 2], K[..., 1, 2], K[..., 0, 0], K[..., 1, 1]
        return cls(torch.stack([2 * cx, 2 * cy, fx, fy, cx, cy], -1))

    @classmethod
    def from_colmap(cls, camera):
        """A COLMAP camera (named tuple or dict with model, width, height, params)."""
        cam = camera._asdict() if hasattr(camera, "_asdict") else camera
        model, params = cam["model"], np.asarray(cam["params"], dtype=np.float64)
        if model in CAMERA_MODELS:
            focal, rest = params[[0, 1, 2, 3]], params[4:]
        elif model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL"):
            focal, rest = params[[0, 0, 1, 2]], params[3:]
            if model == "SIMPLE_RADIAL":
                rest = np.append(rest, 0.0)
        else:
            raise NotImplementedError(model)
        return cls(np.concatenate([[cam["width"], cam["height"]], focal, rest]), model=model)

    @classmethod
    def from_npz(cls, camera):
        """The fork's NPZ camera record: {"model": "OPENCV_FISHEYE", "width", "height", "params": fx fy cx cy k1..k4}."""
        if hasattr(camera, "item") and not isinstance(camera, dict):
            camera = camera.item()
        if str(camera["model"]) != "OPENCV_FISHEYE":
            raise NotImplementedError(f"camera model {camera['model']} in an NPZ record: only OPENCV_FISHEYE")
        params = np.asarray(camera["params"], dtype=np.float32).reshape(-1)
        if params.shape[0] != 8:
            raise ValueError(f"OPENCV_FISHEYE has 8 parameters (fx, fy, cx, cy, k1..k4), got {params.shape[0]}")
        head = np.array([int(camera["width"]), int(camera["height"])], dtype=np.float32)
        return cls(np.concatenate([head, params]), model="OPENCV_FISHEYE")

    size = property(lambda self: self._data[..., :2])
    f = property(lambda self: self._data[..., 2:4])
    c = property(lambda self: self._data[..., 4:6])
    dist = property(lambda self: self._data[..., 6:])

    def scale(self, scales):
        """The camera of the image resized by `scales` (sx, sy)."""
        s = _tensor(scales).to(self._data)
        return self._like(torch.cat([self.size * s, self.f * s, self.c * s, self.dist], -1))

    def crop(self, left_top, size):
        """The camera of the crop [left_top, left_top + size)."""
        lt, sz = self._data.new_tensor(left_top), self._data.new_tensor(size)
        return self._like(torch.cat([sz.expand_as(self.size), self.f, self.c - lt, self.dist], -1))


def model_id(camera):
    """The `int model` of the C ABI.  As in the reference only OPENCV_FISHEYE is told by name; every other model is
    told by the number of coefficients it carries (SIMPLE_RADIAL is stored as RADIAL with k2 = 0)."""
    width = camera._data.shape[-1]
    if getattr(camera, "model", None) == "OPENCV_FISHEYE" and width > 6:
        return GFC_CAM_OPENCV_FISHEYE
    return {6: GFC_CAM_PINHOLE, 8: GFC_CAM_RADIAL, 10: GFC_CAM_OPENCV}[width]


def camera_args(camera, batch, device):
    """Camera-like (`_data`, `model`) -> ([batch,10] fp32 on `device`, missing coefficients zero, and the model id)."""
    data = camera._data.to(device=device, dtype=torch.float32).reshape(-1, camera._data.shape[-1])
    if data.shape[0] == 1 and batch > 1:
        data = data.expand(batch, -1)
    assert data.shape[0] == batch, f"{data.shape[0]} cameras for {batch} pairs"
    out = torch.zeros((batch, 10), device=device, dtype=torch.float32)
    out[:, :data.shape[1]] = data
    return out, model_id(camera)


def pose_args(pose, batch, device):
    """Pose-like (`_data`) or a [..., 4, 4] / [..., 12] tensor -> ([batch,12] fp32 on `device`, its inverse likewise).
    The inverse is formed in fp32 by the expression of `Pose.inv`, like the reference's `T_0to1.inv()`."""
    if isinstance(pose, torch.Tensor):
        pose = Pose.from_4x4mat(pose) if pose.shape[-2:] == (4, 4) else Pose(pose)
    fwd = Pose(pose._data.to(device=device, dtype=torch.float32).reshape(-1, 12))
    assert fwd._data.shape[0] == batch, f"{fwd._data.shape[0]} poses for {batch} pairs"
    return fwd._data.contiguous(), fwd.inv()._data.contiguous()
