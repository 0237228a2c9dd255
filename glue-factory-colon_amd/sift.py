"""SIFT stages on the MI355X (csrc/sift.hip): scale space, detection, orientation, descriptor.

The algorithm is the package's own, stated in float64 in tests/sift_reference.py: Lowe's detector and descriptor with
the meaning pycolmap gives the reference's conf keys (gluefactory/models/extractors/sift.py:139-144).  UNPINNED: the
reference delegates SIFT to OpenCV, pycolmap or CudaSift, none of which is available here -- these are NOT the key
points of any of those libraries, and a checkpoint fine-tuned on one of them sees a different detector.

The stage calls (one function per entry point of include/gfc_amd.h) produce a raw list ordered by (octave, layer, y, x
of the integer extremum, orientation peak by bin); `filter_list` is the reference's post-processing on the device
(specular rule, filter_dog_point, top-k, RootSIFT), `extract` all of it in one library call, and `SIFT` the
`extractors.sift` model with the reference's conf
keys, inputs and outputs (gluefactory/models/extractors/sift.py:97-463), backend "gfc_amd".
"""
import ctypes
from collections import namedtuple

import torch

from . import _native as nat
from ._superpoint_common import joint_pair_data, pad_keypoints_native
from .base_model import BaseModel, conf_get

Octave = namedtuple("Octave", "h w gauss_offset dog_offset")
Layout = namedtuple("Layout", "octaves gauss_floats dog_floats")
N_GAUSS, N_DOG = 6, 5
_ws = nat.Workspace()


def pyramid_layout(h, w, first_octave=-1, num_octaves=4):
    """Where the levels of an H x W batch live (floats, per image): see include/gfc_amd.h."""
    out = (ctypes.c_int64 * 35)()
    nat.call("gfc_sift_pyramid_layout", h, w, first_octave, num_octaves, out)
    octs = [Octave(*(int(out[3 + 4 * o + i]) for i in range(4))) for o in range(int(out[0]))]
    return Layout(octs, int(out[1]), int(out[2]))


def level(buf, layout, b, o, s, dog=False):
    """View of level s of octave o of image b in a `pyramid` output (the padded plane)."""
    oc = layout.octaves[o]
    off = (oc.dog_offset if dog else oc.gauss_offset) + s * oc.h * oc.w
    return buf[b, off: off + oc.h * oc.w].view(oc.h, oc.w)


def _valid(valid_wh, device):
    if valid_wh is None:
        return None
    return valid_wh.to(device=device, dtype=torch.int32).contiguous()


def pyramid(image, valid_wh=None, first_octave=-1, num_octaves=4):
    """image fp32 [B,H,W] -> (gauss [B,gauss_floats], dog [B,dog_floats], layout)."""
    nat.require_cuda(image, "image")
    image = image.contiguous().float()
    b, h, w = image.shape
    lay = pyramid_layout(h, w, first_octave, num_octaves)
    gauss = torch.empty(b, lay.gauss_floats, device=image.device)
    dog = torch.empty(b, lay.dog_floats, device=image.device)
    v = _valid(valid_wh, image.device)
    nat.call("gfc_sift_pyramid", image, b, h, w, v, first_octave, num_octaves, gauss, dog)
    return gauss, dog, lay


def detect(dog, h, w, valid_wh=None, first_octave=-1, num_octaves=4, detection_threshold=0.0066667, edge_threshold=10.0,
           cap=16384):
    """dog [B,dog_floats] of an H x W batch -> (raw_f [B,cap,8], raw_i [B,cap,8], counts [B,4])."""
    nat.require_cuda(dog, "dog")
    b, dev = dog.shape[0], dog.device
    raw_f = torch.zeros(b, cap, 8, device=dev)
    raw_i = torch.zeros(b, cap, 8, dtype=torch.int32, device=dev)
    counts = torch.zeros(b, 4, dtype=torch.int32, device=dev)
    need = nat.call("gfc_sift_detect_workspace_bytes", b, cap)
    ws = _ws.get(need, dev)
    v = _valid(valid_wh, dev)
    nat.call("gfc_sift_detect", dog, b, h, w, v, first_octave, num_octaves, float(detection_threshold),
             float(edge_threshold), cap, raw_f, raw_i, counts, ws, need)
    return raw_f, raw_i, counts


def orient(gauss, h, w, raw_f, raw_i, counts, valid_wh=None, first_octave=-1, num_octaves=4, ocap=None):
    """-> (ori_f [B,ocap,8] with the angle in slot 7, ori_i [B,ocap,4], ocounts [B,2])."""
    nat.require_cuda(gauss, "gauss")
    b, cap, dev = raw_f.shape[0], raw_f.shape[1], gauss.device
    ocap = ocap or 4 * cap  # at most 4 orientations per key point: the default cannot overflow
    ori_f = torch.zeros(b, ocap, 8, device=dev)
    ori_i = torch.zeros(b, ocap, 4, dtype=torch.int32, device=dev)
    ocounts = torch.zeros(b, 2, dtype=torch.int32, device=dev)
    need = nat.call("gfc_sift_orient_workspace_bytes", b, cap)
    ws = _ws.get(need, dev)
    v = _valid(valid_wh, dev)
    nat.call("gfc_sift_orient", gauss, b, h, w, v, first_octave, num_octaves, raw_f, raw_i, counts, cap, ocap, ori_f,
             ori_i, ocounts, ws, need)
    return ori_f, ori_i, ocounts


def describe(gauss, h, w, ori_f, ori_i, ocounts, valid_wh=None, first_octave=-1, num_octaves=4):
    """-> desc [B,ocap,128] (L2, clamp 0.2, L2); rows beyond ocounts[b, 0] are zero."""
    nat.require_cuda(gauss, "gauss")
    b, ocap, dev = ori_f.shape[0], ori_f.shape[1], gauss.device
    desc = torch.zeros(b, ocap, 128, device=dev)
    v = _valid(valid_wh, dev)
    nat.call("gfc_sift_describe", gauss, b, h, w, v, first_octave, num_octaves, ori_f, ori_i, ocounts, ocap, desc)
    return desc


def extract_raw(image, valid_wh=None, first_octave=-1, num_octaves=4, detection_threshold=0.0066667, edge_threshold=10.0,
                cap=4096):
    """The four stages in sequence on the current stream, no host read in between (counts[:, 2] holds the candidates
    beyond cap; the oriented list is sized 4 x cap and cannot overflow).
    -> dict(ori_f, ori_i, ocounts, descriptors, counts): the oriented raw list of every image, before any filtering."""
    b, h, w = image.shape
    gauss, dog, _ = pyramid(image, valid_wh, first_octave, num_octaves)
    raw_f, raw_i, counts = detect(dog, h, w, valid_wh, first_octave, num_octaves, detection_threshold, edge_threshold, cap)
    ori_f, ori_i, ocounts = orient(gauss, h, w, raw_f, raw_i, counts, valid_wh, first_octave, num_octaves)
    desc = describe(gauss, h, w, ori_f, ori_i, ocounts, valid_wh, first_octave, num_octaves)
    return dict(ori_f=ori_f, ori_i=ori_i, ocounts=ocounts, descriptors=desc, counts=counts)


def gray(image):
    """[B,3,H,W] -> [B,H,W]: (image * [0.299, 0.587, 0.114]).sum(1), the package's rgb_to_gray kernel."""
    nat.require_cuda(image, "image")
    image = image.contiguous().float()
    b, _, h, w = image.shape
    out = torch.empty(b, h, w, device=image.device)
    nat.call("gfc_sift_gray", image, out, b, h, w)
    return out


def filter_list(ori_f, desc, ocounts, h, w, valid_wh=None, specular=None, nms_radius=0, scale_weighting=False, k=None,
                rootsift=True, out_cap=None):
    """The reference's post-processing (gfc_sift_filter).  nms_radius None skips filter_dog_point, k None keeps all.
    -> dict(keypoints [B,out_cap,2], scales, oris, keypoint_scores [B,out_cap], descriptors [B,out_cap,128],
    index [B,out_cap] int32 (row of the oriented list, -1 beyond the count), counts [B] int32)."""
    nat.require_cuda(ori_f, "ori_f")
    b, ocap, dev = ori_f.shape[0], ori_f.shape[1], ori_f.device
    kk = int(k) if k else 0
    out_cap = out_cap or (min(kk, ocap) if kk else ocap)
    out = dict(keypoints=torch.zeros(b, out_cap, 2, device=dev), scales=torch.zeros(b, out_cap, device=dev),
               oris=torch.zeros(b, out_cap, device=dev), keypoint_scores=torch.zeros(b, out_cap, device=dev),
               descriptors=torch.zeros(b, out_cap, 128, device=dev),
               index=torch.zeros(b, out_cap, dtype=torch.int32, device=dev),
               counts=torch.zeros(b, dtype=torch.int32, device=dev))
    need = nat.call("gfc_sift_filter_workspace_bytes", b, h, w, ocap)
    ws = _ws.get(need, dev)
    v = _valid(valid_wh, dev)
    if specular is not None:
        specular = specular.to(device=dev).reshape(b, h, w).ne(0).to(torch.uint8).contiguous()
    nat.call("gfc_sift_filter", ori_f, desc, ocounts, b, ocap, h, w, v, specular,
             -1 if nms_radius is None else int(nms_radius), int(bool(scale_weighting)), kk, int(bool(rootsift)), out_cap,
             out["keypoints"], out["scales"], out["oris"], out["keypoint_scores"], out["descriptors"], out["index"],
             out["counts"], ws, need)
    return out


def extract(image, valid_wh=None, specular=None, first_octave=-1, num_octaves=4, detection_threshold=0.0066667,
            edge_threshold=10.0, cap=16384, ocap=None, nms_radius=0, scale_weighting=False, k=None, rootsift=True,
            out_cap=None):
    """All stages in ONE library call (gfc_sift_extract): image fp32 [B,H,W] -> the dict of `filter_list` plus
    stage_counts [B,4] (key points, candidates, candidates beyond cap, 0) and ocounts [B,2]."""
    nat.require_cuda(image, "image")
    image = image.contiguous().float()
    b, h, w = image.shape
    dev = image.device
    ocap = ocap or 4 * cap
    kk = int(k) if k else 0
    out_cap = out_cap or (min(kk, ocap) if kk else ocap)
    out = dict(keypoints=torch.zeros(b, out_cap, 2, device=dev), scales=torch.zeros(b, out_cap, device=dev),
               oris=torch.zeros(b, out_cap, device=dev), keypoint_scores=torch.zeros(b, out_cap, device=dev),
               descriptors=torch.zeros(b, out_cap, 128, device=dev),
               index=torch.zeros(b, out_cap, dtype=torch.int32, device=dev),
               counts=torch.zeros(b, dtype=torch.int32, device=dev),
               stage_counts=torch.zeros(b, 4, dtype=torch.int32, device=dev),
               ocounts=torch.zeros(b, 2, dtype=torch.int32, device=dev))
    need = nat.call("gfc_sift_extract_workspace_bytes", b, h, w, first_octave, num_octaves, cap, ocap)
    if need == 0:
        # the call itself says why (unsupported shape or invalid argument)
        need = 1
    ws = _ws.get(need, dev)
    v = _valid(valid_wh, dev)
    if specular is not None:
        specular = specular.to(device=dev).reshape(b, h, w).ne(0).to(torch.uint8).contiguous()
    nat.call("gfc_sift_extract", image, b, h, w, v, specular, first_octave, num_octaves, float(detection_threshold),
             float(edge_threshold), cap, ocap, -1 if nms_radius is None else int(nms_radius), int(bool(scale_weighting)),
             kk, int(bool(rootsift)), out_cap, out["keypoints"], out["scales"], out["oris"], out["keypoint_scores"],
             out["descriptors"], out["index"], out["counts"], out["stage_counts"], out["ocounts"], ws, need)
    return out


_ABSENT = {"opencv": "cv2 (OpenCV)", "pycolmap": "pycolmap", "pycolmap_cpu": "pycolmap", "pycolmap_cuda": "pycolmap",
           "py_cudasift": "cudasift_py (CudaSift)", "py_Cudasift": "cudasift_py (CudaSift)",
           "py_CudaSift": "cudasift_py (CudaSift)"}


class SIFT(BaseModel):
    """`extractors.sift` on the MI355X.  The conf keys are the reference's (sift.py:98-116); what differs:

    backend                 "gfc_amd" only.  The reference's backends name libraries that are absent here and are refused
                            (NotImplementedError): nothing is substituted silently.
    detection_threshold, edge_threshold, first_octave (-1 or 0), num_octaves: the meaning pycolmap gives them.
    init_blur, filter_kpts_with_wrapper: accepted and ignored (they configure CudaSift).
    random_topk, filter_with_lowest_scale: the score-less ranking branches; this backend always has scores -> refused.
    candidate_cap           MI355X addition: extremum candidates kept per image before refinement; more raise an error
                            that says so (never a silent drop).

    The image is clipped to [0, 1] where the pyramid reads it, as the reference's np.clip does (sift.py:208).
    UNPINNED: not OpenCV's, pycolmap's or CudaSift's key points (see the module docstring)."""

    default_conf = {
        "rootsift": True,
        "nms_radius": 0,  # None: no filter_dog_point at all
        "max_num_keypoints": 4096,
        "backend": "gfc_amd",
        "detection_threshold": 0.0066667,
        "edge_threshold": 10,
        "first_octave": -1,
        "num_octaves": 4,
        "init_blur": 1.0,  # ignored
        "filter_kpts_with_wrapper": True,  # ignored
        "filter_with_scale_weighting": False,  # rank by score x scale
        "extractor_channel": "grayscale",  # or red, green, blue
        "filter_with_lowest_scale": False,  # refused when True
        "force_num_keypoints": False,
        "random_topk": False,  # refused when True
        "mask_out_padded_kpts": False,
        "filter_specular_keypoints": True,
        "candidate_cap": 16384,
    }

    required_data_keys = ["image"]

    def _init(self, conf):
        backend = conf_get(conf, "backend")
        if backend != "gfc_amd":
            if backend in _ABSENT:
                raise NotImplementedError(
                    f"SIFT backend {backend!r} needs {_ABSENT[backend]}, which is not available here; this package only "
                    "has backend 'gfc_amd' (its own detector: not that library's key points)")
            raise ValueError(f"Unknown backend: {backend} not in {{gfc_amd,{','.join(_ABSENT)}}}.")
        if conf_get(conf, "random_topk"):
            raise NotImplementedError("random_topk ranks without scores; backend 'gfc_amd' always has scores")
        if conf_get(conf, "filter_with_lowest_scale"):
            raise NotImplementedError("filter_with_lowest_scale ranks without scores; backend 'gfc_amd' always has scores")
        if conf_get(conf, "extractor_channel") not in ("grayscale", "red", "green", "blue"):
            raise ValueError(f"Unknown extractor_channel: {conf_get(conf, 'extractor_channel')} not in "
                             "{grayscale,red,green,blue}.")
        if conf_get(conf, "force_num_keypoints") and conf_get(conf, "max_num_keypoints") is None:
            raise ValueError("force_num_keypoints needs max_num_keypoints")
        self.set_initialized()

    def _plane(self, image):
        if image.dim() != 4 or image.shape[1] not in (1, 3):
            raise ValueError(f"image must be [B,1|3,H,W], got {tuple(image.shape)}")
        if image.shape[1] == 1:
            return image[:, 0].contiguous().float()
        channel = conf_get(self.conf, "extractor_channel")
        if channel == "grayscale":
            return gray(image)
        return image[:, {"red": 0, "green": 1, "blue": 2}[channel]].contiguous().float()

    @staticmethod
    def _valid_wh(data, b):
        if "image_size" not in data:
            return None
        size = data["image_size"]
        if size.ndim == 1:
            size = size[None].expand(b, 2)
        elif size.ndim == 3:
            size = size[0]
        return size.to(torch.float64).cpu().to(torch.int32)  # int(w), int(h) as in the reference

    def _run(self, data):
        """-> (dict of [B,n_max,...] tensors, per-image counts on the host, core time in ms)."""
        image = data["image"]
        nat.require_cuda(image, "data['image']")
        conf = self.conf
        plane = self._plane(image)
        b, h, w = plane.shape
        valid = self._valid_wh(data, b)
        fo, no = int(conf_get(conf, "first_octave")), int(conf_get(conf, "num_octaves"))
        cap = int(conf_get(conf, "candidate_cap"))
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            start.record()
            gauss, dog, _ = pyramid(plane, valid, fo, no)
            raw_f, raw_i, counts = detect(dog, h, w, valid, fo, no, float(conf_get(conf, "detection_threshold")),
                                          float(conf_get(conf, "edge_threshold")), cap)
            host = counts.cpu()  # the counts the module needs: sizes the oriented list
            if int(host[:, 2].max()) > 0:
                raise RuntimeError(f"SIFT: {int(host[:, 2].max())} extremum candidates beyond candidate_cap = {cap} in one "
                                   "image; raise conf.candidate_cap")
            n_raw = max(int(host[:, 0].max()), 1)
            raw_f, raw_i = raw_f[:, :n_raw].contiguous(), raw_i[:, :n_raw].contiguous()
            ori_f, ori_i, ocounts = orient(gauss, h, w, raw_f, raw_i, counts, valid, fo, no, ocap=4 * n_raw)
            desc = describe(gauss, h, w, ori_f, ori_i, ocounts, valid, fo, no)
            stop.record()
            spec = data.get("specular_mask") if conf_get(conf, "filter_specular_keypoints") else None
            k = conf_get(conf, "max_num_keypoints")
            out = filter_list(ori_f, desc, ocounts, h, w, valid, spec, conf_get(conf, "nms_radius"),
                              conf_get(conf, "filter_with_scale_weighting"), k, conf_get(conf, "rootsift"),
                              out_cap=int(k) if k else None)
            lens = out["counts"].cpu().tolist()
        return out, lens, start.elapsed_time(stop), image

    def _finish(self, out, lens, core_ms, image, data, rows):
        """The reference's output dict for the images `rows` (all of equal count, or padded)."""
        conf = self.conf
        dev = image.device
        sel = {k: out[k][rows] for k in ("keypoints", "scales", "oris", "keypoint_scores", "descriptors")}
        n_b = [lens[i] for i in rows]
        padded = [0] * len(rows)
        if conf_get(conf, "force_num_keypoints"):
            k = int(conf_get(conf, "max_num_keypoints"))
            padded = [k - n for n in n_b]
            sub = {key: data[key][rows] for key in ("image_size",) if key in data and data[key].ndim == 2}
            kp, sc = pad_keypoints_native(sel["keypoints"].contiguous(), sel["keypoint_scores"].contiguous(),
                                          out["counts"][rows].contiguous(), k, 0.0, sub, image)
            sel["keypoints"], sel["keypoint_scores"] = kp, sc
            if conf_get(conf, "mask_out_padded_kpts"):
                sel["valid_depth_keypoints"] = (torch.arange(k, device=dev)[None] < out["counts"][rows][:, None].long())
        else:
            if len(set(n_b)) > 1:
                raise RuntimeError(
                    f"stack expects each tensor to be equal size, but the images kept {n_b} key points: without "
                    "force_num_keypoints a batch of items with differing counts cannot be stacked (as in the reference)")
            n = n_b[0] if n_b else 0
            sel = {key: v[:, :n].contiguous() for key, v in sel.items()}
        sel["num_keypoints_detected"] = torch.tensor(n_b, device=dev)
        sel["num_keypoints_padded"] = torch.tensor(padded, device=dev)
        sel["extractor_core_time_ms"] = torch.full((len(rows),), core_ms / max(len(lens), 1), dtype=torch.float32, device=dev)
        return sel

    def _forward(self, data):
        out, lens, core_ms, image = self._run(data)
        return self._finish(out, lens, core_ms, image, data, list(range(len(lens))))

    def forward_pair(self, data0, data1):
        """Both views of a pair through ONE call when their images agree in shape (MI355X addition used by
        TwoViewPipeline).  Returns (pred0, pred1), each what `self(view)` returns: the counts need only agree inside a
        view."""
        for d in (data0, data1):
            for key in self.required_data_keys:
                assert key in d, f"Missing key {key} in data"
        joint = joint_pair_data(data0, data1)
        if joint is None or ("image_size" in joint and joint["image_size"].ndim != 2):
            return self(data0), self(data1)
        b = data0["image"].shape[0]
        out, lens, core_ms, image = self._run(joint)
        return (self._finish(out, lens, core_ms, image, joint, list(range(b))),
                self._finish(out, lens, core_ms, image, joint, list(range(b, 2 * b))))

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = SIFT
