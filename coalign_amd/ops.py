"""Torch-tensor front end of the C ABI: allocates outputs / workspaces with torch (PyTorch-ROCm owns device
memory and streams), passes raw ``data_ptr()``s and the current stream to the gfx950 kernels.

Every function requires CUDA(ROCm) tensors and raises otherwise -- the hot path has no CPU implementation
in this package (the CPU restatement lives in ``oracle/`` and is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import os as _os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip

FUSE_ATT, FUSE_MAX, FUSE_NONE = 0, 1, 2

# Optional in-pipeline timing: set to a dict to have every op bracket its launches with HIP events recorded on the
# stream the kernels are launched on (bench.py reads the pairs after synchronising).  None = no overhead.
PROFILE = None


def timed(name: str):
    """Bracket a region with HIP events when ``PROFILE`` is active (used by bench.py for the per-stage breakdown)."""
    return _Timed(name)


class _Timed:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        if PROFILE is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e.record()
            PROFILE.setdefault(self.name, []).append((self.s, self.e))
        return False


def _stream() -> ctypes.c_void_p:
    """The current HIP stream of the current device -- which, inside an op, is the device of its tensors (``_device_op``)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_tensor(a) -> Optional[torch.Tensor]:
    """The GPU tensor that places an op's argument ``a`` (``_device_op``): a CUDA tensor itself, the storage of this module's map / buffer types, the first
    such tensor in a list or tuple (``pointwise_heads_split``'s layers, ``warp_fuse_nhwc``'s maps); None for anything on the host."""
    if isinstance(a, DecodeBuffers):
        a = a.counts
    elif isinstance(a, SparseCanvas):
        a = a.feats
    elif isinstance(a, SplitMap):
        a = a.data
    elif isinstance(a, Stage1Store):
        a = a.corners
    elif isinstance(a, PoseGraphArrays):
        a = a.vertices
    elif isinstance(a, (list, tuple)):
        return next((t for t in map(_device_tensor, a) if t is not None), None)
    return a if torch.is_tensor(a) and a.is_cuda else None


def _device_op(fn):
    """Run ``fn`` with the device of its first GPU tensor argument current: outputs / workspaces are allocated there, and the
    kernels go to THAT device's current stream (not to the stream of whatever device happens to be current in the caller)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for a in args:
            a = _device_tensor(a)
            if a is not None:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapper


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _rows_ptr(t: torch.Tensor) -> ctypes.c_void_p:
    """Pointer to the storage position of a (possibly zero-row) row tensor: ``data_ptr()`` of an empty view may be reported as NULL."""
    p = t.data_ptr()
    if p == 0 and t.untyped_storage().nbytes() > 0:
        p = t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()
    return ctypes.c_void_p(p)


def _need_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise hip.CoalignHipError("coalign_amd ops run on the MI355X only: got a CPU tensor (no CPU fallback exists)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _dbl3(v: Sequence[float]):
    return (ctypes.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))


@_device_op
def pillar_vfe_scatter(voxel_features: torch.Tensor, voxel_num_points: torch.Tensor, voxel_coords: torch.Tensor,
                       weight: torch.Tensor, bias: Optional[torch.Tensor], bn: Optional[Tuple[torch.Tensor, ...]], bn_eps: float,
                       use_absolute_xyz: bool, with_distance: bool, voxel_size: Sequence[float], range_min: Sequence[float],
                       n_agents: int, ny: int, nx: int, channels_last: bool = False,
                       canvas_cache: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (pillar_features [M, C], canvas [n_agents, C, ny, nx]).  ``bn`` = (weight, bias, running_mean, running_var).
    ``channels_last``: the canvas comes back in NHWC memory (same logical shape), see coalign_pillar_vfe_scatter_nhwc;
    ``canvas_cache`` (channels-last only): a dict the caller keeps; the canvas is then a PERSISTENT tensor (one per device, stream and
    shape) of which only the rows the previous call wrote are cleared -- 10 MB instead of a 180 MB memset, two launches per frame
    (coalign_pillar_encode_persistent) -- and which the next call with the same cache on the same stream overwrites: for callers that
    consume the canvas before they encode the next frame.  (Also measured and rejected: the memset on a side stream next to the VALU-bound
    encoder -- 71 vs 64 us for the op and 212 vs 250 frames/s for the pipeline; cross-stream events cost more than the overlap wins.)"""
    _need_gpu(voxel_features, voxel_num_points, voxel_coords, weight)
    L = hip.lib()
    vf = _f32c(voxel_features)
    M, P = vf.shape[0], vf.shape[1]
    if vf.dim() != 3 or vf.shape[2] != 4:
        raise ValueError(f"voxel_features must be [M, P, 4], got {tuple(vf.shape)}")
    npts = voxel_num_points.to(torch.int32).contiguous()
    coords = voxel_coords.to(torch.int32).contiguous()
    w = _f32c(weight)
    C = w.shape[0]
    dev = vf.device
    feats = torch.empty((M, C), dtype=torch.float32, device=dev)
    channels_last = bool(channels_last) and P <= 32 and C <= 64 and C > 1 and ny * nx > 1
    entry = None
    if channels_last and canvas_cache is not None and C % 4 == 0:
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, n_agents, C, ny, nx)
        entry = canvas_cache.get(key)
        if entry is None or entry["M"] < 0:              # first use (or a failed call before): a zeroed canvas, an all -1 cell map
            entry = canvas_cache[key] = {"canvas": torch.empty((n_agents, C, ny, nx), dtype=torch.float32, device=dev, memory_format=torch.channels_last).zero_(),
                                         "cellmap": torch.full((n_agents * ny * nx,), -1, dtype=torch.int32, device=dev),
                                         "dest": torch.empty(max(M, 1), dtype=torch.int32, device=dev), "M": 0}
        canvas = entry["canvas"]
    else:
        canvas = torch.empty((n_agents, C, ny, nx), dtype=torch.float32, device=dev,
                             memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    bnp = [None] * 4 if bn is None else [_f32c(t) for t in bn]
    b = None if bias is None else _f32c(bias)
    args = (_ptr(vf), _ptr(npts), _ptr(coords), M, P, _ptr(w), _ptr(b), _ptr(bnp[0]), _ptr(bnp[1]), _ptr(bnp[2]), _ptr(bnp[3]), float(bn_eps), C,
            int(use_absolute_xyz), int(with_distance), _dbl3(voxel_size), _dbl3(range_min), n_agents, ny, nx, _ptr(feats))
    with _Timed("pillar_vfe_scatter"):
        if entry is not None:
            need = max(M, entry["M"], 1)
            if entry["dest"].numel() < need:
                grown = torch.empty(need, dtype=torch.int32, device=dev)
                grown[: entry["dest"].numel()] = entry["dest"]
                entry["dest"] = grown
            m_prev, entry["M"] = entry["M"], -1            # an exception below leaves the entry marked unusable
            hip.check(L.coalign_pillar_encode_persistent(*args, _ptr(entry["dest"]), m_prev, _ptr(canvas), _ptr(entry["cellmap"]), _stream()),
                      "coalign_pillar_encode_persistent")
            entry["M"] = M
        else:
            ws_bytes = L.coalign_pillar_scatter_workspace_bytes(n_agents, ny, nx)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            fn = L.coalign_pillar_vfe_scatter_nhwc if channels_last else L.coalign_pillar_vfe_scatter
            hip.check(fn(*args, _ptr(canvas), _ptr(ws), ws_bytes, _stream()), "coalign_pillar_vfe_scatter")
    return feats, canvas


@_device_op
def pillar_encode_stream(voxel_features: torch.Tensor, voxel_num_points: torch.Tensor, voxel_coords: torch.Tensor, count_dev: torch.Tensor,
                         weight: torch.Tensor, bias: Optional[torch.Tensor], bn: Optional[Tuple[torch.Tensor, ...]], bn_eps: float,
                         use_absolute_xyz: bool, with_distance: bool, voxel_size: Sequence[float], range_min: Sequence[float],
                         n_agents: int, ny: int, nx: int, canvas_cache: dict, unique_cells: bool = True,
                         want_features: bool = False) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """The persistent-canvas encoder behind a producer that keeps its pillar count on the device (``ops.voxelize``): the arrays are
    capacity sized, ``count_dev`` (int32 device tensor, first element) says how many rows are valid; nothing here reads it on the host, so
    voxeliser -> encoder -> backbone is one stream of launches (one captured graph).  ``canvas_cache``: as in ``pillar_vfe_scatter`` (one
    persistent channels-last canvas per device, stream and shape).  -> (pillar_features [capacity, C] or None, canvas [n_agents, C, ny, nx])."""
    _need_gpu(voxel_features, voxel_num_points, voxel_coords, count_dev, weight)
    L = hip.lib()
    vf = _f32c(voxel_features)
    cap, P = vf.shape[0], vf.shape[1]
    if vf.dim() != 3 or vf.shape[2] != 4:
        raise ValueError(f"voxel_features must be [M, P, 4], got {tuple(vf.shape)}")
    if count_dev.dtype != torch.int32:
        raise ValueError("count_dev must be an int32 device tensor")
    npts = voxel_num_points.to(torch.int32).contiguous()
    coords = voxel_coords.to(torch.int32).contiguous()
    w = _f32c(weight)
    C = w.shape[0]
    dev = vf.device
    if P > 32 or C > 64 or C % 4:
        raise hip.CoalignHipError("pillar_encode_stream: the channels-last encoder needs P <= 32 and C <= 64 (a multiple of 4)")
    # (the capacity is part of the key: the C entry point clears "the rows the previous call wrote" out of a slot list of THIS capacity -- a smaller
    #  capacity on the same canvas would leave the previous frame's rows beyond it uncleared)
    key = ("stream", str(dev), torch.cuda.current_stream(dev).cuda_stream, n_agents, C, ny, nx, bool(unique_cells), int(cap))
    entry = canvas_cache.get(key)
    if entry is None:
        entry = canvas_cache[key] = {
            "canvas": torch.empty((n_agents, C, ny, nx), dtype=torch.float32, device=dev, memory_format=torch.channels_last).zero_(),
            "cellmap": None if unique_cells else torch.full((n_agents * ny * nx,), -1, dtype=torch.int32, device=dev),
            "dest": torch.zeros(cap + 1, dtype=torch.int32, device=dev)}
    canvas = entry["canvas"]
    feats = torch.empty((cap, C), dtype=torch.float32, device=dev) if want_features else None
    bnp = [None] * 4 if bn is None else [_f32c(t) for t in bn]
    b = None if bias is None else _f32c(bias)
    with _Timed("pillar_encode_stream"):
        hip.check(L.coalign_pillar_encode_stream(_ptr(vf), _ptr(npts), _ptr(coords), cap, _ptr(count_dev), P, _ptr(w), _ptr(b), _ptr(bnp[0]), _ptr(bnp[1]),
                                                 _ptr(bnp[2]), _ptr(bnp[3]), float(bn_eps), C, int(use_absolute_xyz), int(with_distance), _dbl3(voxel_size),
                                                 _dbl3(range_min), n_agents, ny, nx, _ptr(feats), _ptr(entry["dest"]), _ptr(canvas), _ptr(entry["cellmap"]),
                                                 int(bool(unique_cells)), _stream()), "coalign_pillar_encode_stream")
    return feats, canvas


_SP_RANGE_FLAGS: dict = {}


def sp_range_flag(device, create: bool = True) -> Optional[torch.Tensor]:
    """The device word every SplitMap-producing kernel ORs bit 0 into when a value left the pair's range (|x| > 65504; include/coalign_amd.h (9e)).  One per
    device, never cleared by the kernels.  Created on first use outside a graph capture (``FramePipeline`` creates it before capturing); ``None`` if it does not
    exist yet and ``create`` is false or a capture is running (the kernels then skip the report)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    f = _SP_RANGE_FLAGS.get(key)
    if f is None and create and not torch.cuda.is_current_stream_capturing():
        f = _SP_RANGE_FLAGS[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return f


def sp_range_exceeded(device, clear: bool = True) -> bool:
    """True if a SplitMap value exceeded the fp16 split's operating range since the last clearing call (synchronises the device)."""
    f = sp_range_flag(device, create=False)
    if f is None:
        return False
    hit = bool(int(f.item()) & 1)
    if hit and clear:
        f.zero_()
    return hit


class SplitMap:
    """An activation map stored as sp16 pairs in the matrix instructions' operand order (csrc/conv3x3_sp.hip, include/coalign_amd.h (9e)): what the 3x3
    convolutions of the fp16 mode hand to each other inside a ResNet stage.  ``shape`` is the logical [N, C, H, W]; ``data`` the float16 tensor
    [N, C / 16, 4, H, W, 8] (plane = 2 * channel half + term); ``dense()`` returns the float32 tensor the pairs stand for (the values rounded to 22 bits)."""

    def __init__(self, data: torch.Tensor):
        if data.dtype != torch.float16 or data.dim() != 6 or data.shape[2] != 4 or data.shape[5] != 8 or not data.is_contiguous():
            raise ValueError("SplitMap data: contiguous float16 [N, C / 16, 4, H, W, 8]")
        self.data = data
        self.shape = (data.shape[0], data.shape[1] * 16, data.shape[3], data.shape[4])
        self.device, self.dtype, self.is_cuda = data.device, torch.float32, data.is_cuda

    @staticmethod
    def empty(N: int, C: int, H: int, W: int, device) -> "SplitMap":
        if C % 16:
            raise ValueError("SplitMap: C % 16 == 0")
        return SplitMap(torch.empty((N, C // 16, 4, H, W, 8), dtype=torch.float16, device=device))

    @staticmethod
    def pack(x: torch.Tensor) -> "SplitMap":
        """float32 [N, C, H, W] (NCHW or channels-last memory) -> SplitMap (``coalign_sp_pack``)."""
        _need_gpu(x)
        nhwc = x.dtype == torch.float32 and is_channels_last(x)
        xc = x if nhwc else _f32c(x)
        N, C, H, W = xc.shape
        out = SplitMap.empty(N, C, H, W, xc.device)
        hip.check(hip.lib().coalign_sp_pack(_ptr(xc), int(nhwc), _ptr(out.data), N, C, H, W, _ptr(sp_range_flag(xc.device)), _stream()), "coalign_sp_pack")
        return out

    def dense(self, channels_last: bool = False) -> torch.Tensor:
        N, C, H, W = self.shape
        y = torch.empty((N, C, H, W), dtype=torch.float32, device=self.device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        if channels_last and not nhwc_memory(y):
            y = torch.empty((N, H, W, C), dtype=torch.float32, device=self.device).permute(0, 3, 1, 2)
        hip.check(hip.lib().coalign_sp_unpack(_ptr(self.data), _ptr(y), int(channels_last), N, C, H, W, _stream()), "coalign_sp_unpack")
        return y

    def dense_reference(self) -> torch.Tensor:
        """The same values computed with torch ops from ``data`` (tests: the layout's definition, independent of the unpack kernel)."""
        d = self.data.float()
        v = d[:, :, 0::2] + d[:, :, 1::2] / 1024.0                    # [N, C/16, 2 halves, H, W, 8]
        N, C, H, W = self.shape
        return v.permute(0, 1, 2, 5, 3, 4).reshape(N, C, H, W)


class SparseCanvas:
    """The BEV canvas of one batch as the sparse pair (feature rows, cell stamps) of csrc/pillar_sparse.hip instead of a dense tensor: what
    ``PillarVFE`` + ``PointPillarScatter`` hand to the first ResNet stage on the fast path.  ``shape`` is the dense tensor's; ``dense()`` materialises it
    (the reference's ``spatial_features``) for anyone who needs the tensor."""

    def __init__(self, feats, stamps, state, coords, n_agents, C, ny, nx, count_dev=None, owner: Optional[dict] = None):
        self.feats, self.stamps, self.state, self.coords = feats, stamps, state, coords
        # every canvas of one (device, stream, grid) shares ONE stamp map, and only the LATEST encode through it is in the stamps: `owner` is that map's cache
        # entry, `generation` the encode this object came from.  The consumers refuse a canvas that a later encode has overwritten (check_current) instead of
        # reading the newer frame's rows out of this object's `feats`; on the device a stamp naming a row beyond `feats` reads as empty (M_rows, (9d) / (10b)).
        self.owner, self.generation = owner, None if owner is None else owner.get("generation")
        if feats.numel() == 0 and feats.untyped_storage().nbytes() == 0:      # the consumers take a non-NULL row pointer even when every stamp is stale
            self.feats = torch.empty((1, C), dtype=torch.float32, device=feats.device)[:0]
        self.n_agents, self.C, self.ny, self.nx, self.count_dev = n_agents, C, ny, nx, count_dev
        self.shape = (n_agents, C, ny, nx)
        self.device, self.dtype = feats.device, feats.dtype
        self.is_cuda = True

    def check_current(self) -> None:
        if self.owner is not None and self.owner.get("generation") != self.generation:
            raise hip.CoalignHipError("stale SparseCanvas: a later pillar_encode_sparse on the same device, stream and grid has overwritten the shared stamp map "
                                      "(consume a canvas -- or .dense() it -- before the next encode, or encode on another stream / with another canvas_cache)")

    def dense(self) -> torch.Tensor:
        if self.coords is None:
            raise hip.CoalignHipError("a SparseCanvas encoded through a frame record has no coordinate array of its own: densify from the frame's voxel_coords")
        if self.count_dev is not None:
            m = int(self.count_dev[0].item())
            return scatter_to_bev(self.feats[:m], self.coords[:m], self.n_agents, self.ny, self.nx)
        return scatter_to_bev(self.feats, self.coords, self.n_agents, self.ny, self.nx)


# The frame tag of a sparse canvas is 32 bits and stamps are ordered by (tag, row) through atomicMax: a tag that wrapped would lose against the stale stamps of
# the frames before it.  A stamp map is therefore re-zeroed (stamps + frame words, on the launching stream) after this many launches -- 2^31 frames are 50 days
# of one lane at 500 frames/s; callers that replay a captured launch count the replays themselves (FramePipeline does) and call reset_sparse_canvases.
SPARSE_TAG_RESET_AFTER = 1 << 31


def reset_sparse_canvases(canvas_cache: dict) -> int:
    """Zero the stamps and frame words of every sparse canvas of ``canvas_cache`` on the current stream; -> number of canvases reset."""
    n = 0
    for key, entry in canvas_cache.items():
        if isinstance(key, tuple) and key and key[0] == "sparse":
            entry["stamps"].zero_()
            entry["state"].zero_()
            entry["calls"] = 0
            entry["generation"] = entry.get("generation", 0) + 1      # canvases encoded before the reset are gone
            n += 1
    return n


@_device_op
def pillar_fold_params(weight: torch.Tensor, bias: Optional[torch.Tensor], bn: Optional[Tuple[torch.Tensor, ...]], bn_eps: float, use_absolute_xyz: bool) -> torch.Tensor:
    """The encoder's channel parameters in the form ``pillar_encode_sparse`` uses (include/coalign_amd.h (1b)): once per weight set, like the split
    weight images of the convolutions."""
    _need_gpu(weight)
    L = hip.lib()
    w = _f32c(weight)
    out = torch.empty(L.coalign_pillar_folded_param_bytes() // 4, dtype=torch.float32, device=w.device)
    bnp = [None] * 4 if bn is None else [_f32c(t) for t in bn]
    b = None if bias is None else _f32c(bias)
    hip.check(L.coalign_pillar_fold_params(_ptr(w), _ptr(b), _ptr(bnp[0]), _ptr(bnp[1]), _ptr(bnp[2]), _ptr(bnp[3]), float(bn_eps), w.shape[0], int(use_absolute_xyz),
                                           _ptr(out), _stream()), "coalign_pillar_fold_params")
    return out


class FrameRecordUnsupported(hip.CoalignHipError):
    """The configured route cannot read its inputs through a ``PillarFrameRecord``; the caller copies the frame into the graph's buffers instead."""


class PillarFrameRecord:
    """``coalign_pillar_frame`` (include/coalign_amd.h (1c)) for a replayed graph: ``words`` is a 4-word int64 DEVICE view (array pointers | pillar count) the
    pillar launch reads when it starts, ``host`` the pinned words the owner fills per frame (``set``) and copies over as part of ONE small host-to-device
    transfer.  ``capacity`` sizes the launch; a frame may hold fewer pillars, never more."""

    def __init__(self, words: torch.Tensor, host: torch.Tensor, capacity: int):
        if words.dtype != torch.int64 or words.numel() != 4 or not words.is_cuda or host.dtype != torch.int64 or host.numel() != 4:
            raise ValueError("a frame record is four int64 words on the device and four on the (pinned) host")
        self.words, self.host, self.capacity = words, host, int(capacity)
        self._host_np = host.numpy()

    @staticmethod
    def admits(vf: torch.Tensor, npts: torch.Tensor, coords: torch.Tensor, device) -> bool:
        """The arrays are read IN PLACE: float32 / int32, contiguous, on the launch's device (anything else takes the copying route)."""
        return (vf.is_cuda and vf.device == device and npts.device == device and coords.device == device and vf.dtype == torch.float32 and vf.dim() == 3
                and vf.shape[2] == 4 and npts.dtype == torch.int32 and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
                and vf.is_contiguous() and npts.is_contiguous() and coords.is_contiguous() and npts.shape[0] == vf.shape[0] == coords.shape[0])

    def set(self, vf: torch.Tensor, npts: torch.Tensor, coords: torch.Tensor) -> None:
        M = int(vf.shape[0])
        if M > self.capacity:
            raise ValueError(f"{M} pillars in a frame record of capacity {self.capacity}")
        self._host_np[:] = (_rows_ptr(vf).value or 0, _rows_ptr(npts).value or 0, _rows_ptr(coords).value or 0, M)      # (little endian: the count is the low half of word 3)


@_device_op
def pillar_encode_sparse(voxel_features: torch.Tensor, voxel_num_points: torch.Tensor, voxel_coords: torch.Tensor, weight: torch.Tensor,
                         bias: Optional[torch.Tensor], bn: Optional[Tuple[torch.Tensor, ...]], bn_eps: float, use_absolute_xyz: bool,
                         voxel_size: Sequence[float], range_min: Sequence[float], n_agents: int, ny: int, nx: int, canvas_cache: dict,
                         count_dev: Optional[torch.Tensor] = None, folded: Optional[torch.Tensor] = None, frame: Optional[PillarFrameRecord] = None) -> SparseCanvas:
    """PillarVFE + PointPillarScatter in ONE launch (include/coalign_amd.h (1b)): feature rows [M, C] + 8-byte cell stamps.  ``canvas_cache`` keeps the
    stamp map and the frame-tag words of this (device, stream, grid): they persist across frames and are never cleared (a stamp is valid only with
    the current tag).  ``count_dev``: optional int32 device tensor holding the pillar count (capacity-sized arrays).  ``folded``: ``pillar_fold_params``
    of the same weights; a caller that keeps none gets them folded here (one more small launch per call).  ``frame``: the launch reads its three arrays and the
    count through this device record (include/coalign_amd.h (1c)); the tensors passed here then only give the shapes."""
    _need_gpu(voxel_features, voxel_num_points, voxel_coords, weight)
    L = hip.lib()
    vf = _f32c(voxel_features)
    if vf.dim() != 3 or vf.shape[2] != 4:
        raise ValueError(f"voxel_features must be [M, P, 4], got {tuple(vf.shape)}")
    M, P = vf.shape[0], vf.shape[1]
    if frame is not None:
        if count_dev is not None:
            raise ValueError("a frame record carries the pillar count itself")
        M, npts, coords = frame.capacity, None, None
    else:
        npts = voxel_num_points.to(torch.int32).contiguous()
        coords = voxel_coords.to(torch.int32).contiguous()
    C = weight.shape[0]
    dev = vf.device
    if P > 32 or C > 64:
        raise hip.CoalignHipError("pillar_encode_sparse: P <= 32 and C <= 64")
    if folded is None:
        folded = pillar_fold_params(weight, bias, bn, bn_eps, use_absolute_xyz)
    if folded.dtype != torch.float32 or folded.numel() * 4 != L.coalign_pillar_folded_param_bytes() or folded.device != dev:
        raise ValueError("folded: the tensor pillar_fold_params returned for these weights")
    key = ("sparse", str(dev), torch.cuda.current_stream(dev).cuda_stream, n_agents, ny, nx)
    entry = canvas_cache.get(key)
    if entry is None:
        entry = canvas_cache[key] = {"stamps": torch.zeros(n_agents * ny * nx, dtype=torch.int64, device=dev), "state": torch.zeros(L.coalign_sparse_canvas_state_bytes() // 4, dtype=torch.int32, device=dev)}
    entry["calls"] = entry.get("calls", 0) + 1
    entry["generation"] = entry.get("generation", 0) + 1      # (SparseCanvas.check_current)
    if entry["calls"] >= SPARSE_TAG_RESET_AFTER:             # (never inside a captured frame: a capture happens in a map's first calls)
        entry["stamps"].zero_()
        entry["state"].zero_()
        entry["calls"] = 1
    feats = torch.empty((max(M, 1), C), dtype=torch.float32, device=dev)[:M]      # (an empty frame still hands its consumers a valid row pointer: ADVICE r04)
    if frame is not None:
        with _Timed("pillar_encode_sparse"):
            hip.check(L.coalign_pillar_encode_sparse_frame(_ptr(frame.words), M, P, _ptr(folded), C, int(use_absolute_xyz), _dbl3(voxel_size), _dbl3(range_min), n_agents,
                                                           ny, nx, _ptr(feats), _ptr(entry["stamps"]), _ptr(entry["state"]), _stream()), "coalign_pillar_encode_sparse_frame")
        sc = SparseCanvas(feats, entry["stamps"], entry["state"], None, n_agents, C, ny, nx, None, owner=entry)
        sc.count_word = frame.words[3:4].view(torch.int32)[0:1]      # the record's pillar count (little endian: the low half of word 3), for sp_pack_rows
        return sc
    with _Timed("pillar_encode_sparse"):
        hip.check(L.coalign_pillar_encode_sparse(_ptr(vf), _ptr(npts), _ptr(coords), M, _ptr(count_dev), P, _ptr(folded), C, int(use_absolute_xyz), _dbl3(voxel_size),
                                                 _dbl3(range_min), n_agents, ny, nx, _ptr(feats), _ptr(entry["stamps"]), _ptr(entry["state"]), _stream()),
                  "coalign_pillar_encode_sparse")
    return SparseCanvas(feats, entry["stamps"], entry["state"], coords, n_agents, C, ny, nx, count_dev, owner=entry)


@_device_op
def conv3x3_emu_sparse(sc: SparseCanvas, w_split: torch.Tensor, bias: torch.Tensor, cout: int, relu: bool, terms: int, out_channels_last: bool, out_split: bool = False):
    """The strided first convolution of the backbone reading a SparseCanvas (include/coalign_amd.h (9d)); tap-pair weight image.  ``out_split`` (terms 16):
    the result is a ``SplitMap`` (the input of ``conv3x3_sp``)."""
    L = hip.lib()
    sc.check_current()
    N, Cin, H, W = sc.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if w_split.numel() != L.coalign_conv3x3_emu_weight_bytes(Cin, cout, terms):
        raise ValueError("split weight image does not match (Cin, Cout, terms)")
    if out_split:
        if terms != 16:
            raise ValueError("SplitMap outputs belong to the fp16 split (terms = 16)")
        out = SplitMap.empty(N, cout, Ho, Wo, sc.device)
        y = out.data
    else:
        out = y = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=sc.device, memory_format=torch.channels_last if out_channels_last else torch.contiguous_format)
    with _Timed("conv3x3_emu_sparse"):
        hip.check(L.coalign_conv3x3_emu_sparse(_rows_ptr(sc.feats), int(sc.feats.shape[0]), _ptr(sc.stamps), _ptr(sc.state), _ptr(w_split), _ptr(_f32c(bias)), _ptr(y), N, Cin, cout, H, W,
                                               int(relu), terms, 2 if out_split else int(out_channels_last), _ptr(sp_range_flag(sc.device)) if out_split else None, _stream()),
                  "coalign_conv3x3_emu_sparse")
    return out


@_device_op
def pointwise_conv_sparse(sc: SparseCanvas, w_emu: torch.Tensor, bias: torch.Tensor, cout: int, relu: bool, out_channels_last: bool) -> torch.Tensor:
    """The 1 x 1 / stride-2 skip convolution reading a SparseCanvas (include/coalign_amd.h (10b)); ``w_emu``: ``pack_pointwise_emu_weight`` image."""
    L = hip.lib()
    sc.check_current()
    N, Cin, H, W = sc.shape
    if w_emu.dtype != torch.int16 or w_emu.dim() != 5 or w_emu.shape[1] * 16 != Cin:
        raise ValueError("pointwise_conv_sparse needs the split-bf16 weight image of this Cin")
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=sc.device, memory_format=torch.channels_last if out_channels_last else torch.contiguous_format)
    with _Timed("pointwise_conv_sparse"):
        hip.check(L.coalign_pointwise_conv_emu_sparse(_rows_ptr(sc.feats), int(sc.feats.shape[0]), _ptr(sc.stamps), _ptr(sc.state), _ptr(w_emu), _ptr(_f32c(bias)), _ptr(y), N, Cin, H, W, cout,
                                                      w_emu.shape[0] * 32, int(relu), int(out_channels_last), _stream()), "coalign_pointwise_conv_emu_sparse")
    return y


@_device_op
def scatter_to_bev(pillar_features: torch.Tensor, voxel_coords: torch.Tensor, n_agents: int, ny: int, nx: int) -> torch.Tensor:
    """pillar_features [M, C] + coords (agent, z, y, x) -> canvas [n_agents, C, ny, nx]."""
    _need_gpu(pillar_features, voxel_coords)
    L = hip.lib()
    pf = _f32c(pillar_features)
    coords = voxel_coords.to(torch.int32).contiguous()
    M, C = pf.shape
    canvas = torch.empty((n_agents, C, ny, nx), dtype=torch.float32, device=pf.device)
    ws_bytes = L.coalign_pillar_scatter_workspace_bytes(n_agents, ny, nx)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pf.device)
    hip.check(L.coalign_scatter_to_bev(_ptr(pf), _ptr(coords), M, C, n_agents, ny, nx, _ptr(canvas), _ptr(ws), ws_bytes, _stream()),
              "coalign_scatter_to_bev")
    return canvas


@_device_op
def warp_fuse(x: torch.Tensor, theta: torch.Tensor, group_len: Sequence[int], mode: int,
              out_hw: Optional[Tuple[int, int]] = None, rows: Optional[Sequence[int]] = None) -> torch.Tensor:
    """x [n_total, C, H, W] f32, theta [n_total, 2, 3] f64 (device) -> fused [len(group_len), C, Ho, Wo]
    (or [n_total, C, Ho, Wo] for FUSE_NONE).  ``rows``: per frame, the row of x holding logical agent i (default identity)."""
    _need_gpu(x, theta)
    L = hip.lib()
    xc = _f32c(x)
    th = theta.to(device=xc.device, dtype=torch.float64).contiguous()
    n_total, C, H, W = xc.shape
    Ho, Wo = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    groups = [int(g) for g in group_len]
    n_out = n_total if mode == FUSE_NONE else len(groups)
    out = torch.empty((n_out, C, Ho, Wo), dtype=torch.float32, device=xc.device)
    gl = (ctypes.c_int32 * max(1, len(groups)))(*groups)
    rw = None
    if rows is not None:
        if len(rows) != n_total:
            raise ValueError("rows must have one entry per agent")
        rw = (ctypes.c_int32 * max(1, n_total))(*[int(r) for r in rows])
    with _Timed(f"warp_fuse_C{C}"):
        hip.check(L.coalign_warp_fuse_rows(_ptr(xc), n_total, C, H, W, _ptr(th), gl, len(groups), rw, mode, _ptr(out), Ho, Wo, _stream()),
                  "coalign_warp_fuse_rows")
    return out


@_device_op
def normalize_pairwise(pairwise_t_matrix: torch.Tensor, H: int, W: int, den_x: float, den_y: float) -> torch.Tensor:
    """[..., 4, 4] float64 (device) -> [..., 2, 3] float64: normalize_pairwise_tfm in one launch (include/coalign_amd.h)."""
    _need_gpu(pairwise_t_matrix)
    t = pairwise_t_matrix.contiguous()
    if t.dtype != torch.float64 or t.shape[-2:] != (4, 4):
        raise ValueError("pairwise_t_matrix must be float64 [..., 4, 4]")
    out = torch.empty(tuple(t.shape[:-2]) + (2, 3), dtype=torch.float64, device=t.device)
    n = t.numel() // 16
    hip.check(hip.lib().coalign_normalize_pairwise(_ptr(t), n, int(H), int(W), float(den_x), float(den_y), _ptr(out), _stream()),
              "coalign_normalize_pairwise")
    return out


def warp_fuse_nhwc_ok(x: torch.Tensor) -> bool:
    """Channels-last map the one-launch fusion kernel serves: [n <= 8, C in {64, 128, 256}, H, W] float32 in NHWC memory."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] in (64, 128, 256) and x.shape[0] <= 8 and is_channels_last(x)


@_device_op
def warp_fuse_nhwc(xs: Sequence[torch.Tensor], theta: torch.Tensor, mode: int, rows: Optional[Sequence[int]] = None,
                   out_hw: Optional[Sequence[Tuple[int, int]]] = None) -> list:
    """Up to three channels-last feature scales of ONE frame, ``xs[i]`` [n, C_i, H_i, W_i] (NHWC memory), theta [n, 2, 3] f64 ->
    per scale the fused map [1, C_i, Ho_i, Wo_i] (ATT / MAX) or the warped maps [n, C_i, Ho_i, Wo_i] (NONE), channels-last."""
    _need_gpu(*xs, theta)
    L = hip.lib()
    k = len(xs)
    n = xs[0].shape[0]
    if not 1 <= k <= 3 or any(not warp_fuse_nhwc_ok(x) or x.shape[0] != n for x in xs):
        raise ValueError("warp_fuse_nhwc needs 1-3 channels-last float32 maps [n <= 8, C in {64, 128, 256}, H, W] of one frame")
    th = theta.to(device=xs[0].device, dtype=torch.float64).contiguous()
    if th.shape[0] != n:
        raise ValueError("one theta row per agent")
    hw = [tuple(x.shape[2:]) for x in xs] if out_hw is None else [(int(a), int(b)) for a, b in out_hw]
    outs = [torch.empty((n if mode == FUSE_NONE else 1, x.shape[1], h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            for x, (h, w) in zip(xs, hw)]
    vp = ctypes.c_void_p * k
    i32 = ctypes.c_int32 * k
    rw = None
    if rows is not None:
        if len(rows) != n:
            raise ValueError("rows must have one entry per agent")
        rw = (ctypes.c_int32 * n)(*[int(r) for r in rows])
    with _Timed("warp_fuse_nhwc"):
        hip.check(L.coalign_warp_fuse_nhwc(k, vp(*[x.data_ptr() for x in xs]), i32(*[x.shape[1] for x in xs]), i32(*[x.shape[2] for x in xs]),
                                           i32(*[x.shape[3] for x in xs]), vp(*[o.data_ptr() for o in outs]), i32(*[h for h, _ in hw]),
                                           i32(*[w for _, w in hw]), n, _ptr(th), rw, mode, _stream()), "coalign_warp_fuse_nhwc")
    return outs


class DecodeBuffers:
    """Caller-owned candidate buffers + workspaces of the post-processing kernels (reused across frames)."""

    def __init__(self, capacity: int, A: int, H: int, W: int, top: int, device):
        L = hip.lib()
        self.capacity, self.top = capacity, top
        self.dec_A, self.dec_HW = A, (H, W)
        self.frame_words = torch.zeros(67, dtype=torch.int32, device=device)  # cleared once per frame by ONE launch (reset_frame); copied to the host as ONE block
        self.counts = self.frame_words[:64]                                    # chained per-agent totals
        self.status = self.frame_words[64:65]
        self.cand_index = torch.empty(capacity, dtype=torch.int32, device=device)
        self.cand_score = torch.empty(capacity, dtype=torch.float32, device=device)
        self.cand_box7 = torch.empty((capacity, 7), dtype=torch.float32, device=device)
        self.cand_corners = torch.empty((capacity, 8, 3), dtype=torch.float32, device=device)
        self.cand_keep = torch.empty(capacity, dtype=torch.uint8, device=device)
        self.dec_ws_bytes = L.coalign_anchor_decode_workspace_bytes(A, H, W)
        self.dec_ws = torch.empty(max(1, self.dec_ws_bytes), dtype=torch.uint8, device=device)
        self.nms_ws_bytes = L.coalign_nms_rotated_workspace_bytes(capacity, top)
        self.nms_ws = torch.empty(max(1, self.nms_ws_bytes), dtype=torch.uint8, device=device)
        self.keep = torch.empty(top, dtype=torch.int32, device=device)
        self.keep_count = self.frame_words[65:66]
        self.out_flat = torch.empty(top * 25, dtype=torch.float32, device=device)      # corners | scores in ONE allocation: a finished frame is taken out with one copy launch
        self.out_corners = self.out_flat[: top * 24].view(top, 8, 3)
        self.out_scores = self.out_flat[top * 24:]
        self.out_count = self.frame_words[66:67]
        self.host = torch.zeros(67, dtype=torch.int32).pin_memory()  # the frame words of the last frame: chained totals | status | kept | final


    def reset_frame(self) -> None:
        """counts / status of a new frame: one hand-written fill launch on the current stream (no torch fill in the captured frame)."""
        with torch.cuda.device(self.frame_words.device):
            hip.check(hip.lib().coalign_fill_words(_ptr(self.frame_words), self.frame_words.numel(), 0, _stream()), "coalign_fill_words")


@_device_op
def anchor_decode(buf: DecodeBuffers, slot: int, cls: torch.Tensor, reg: torch.Tensor, dir_: Optional[torch.Tensor],
                  anchors_f32: torch.Tensor, score_thr: float, dir_offset: float, num_bins: int, order: str,
                  transform: Optional[torch.Tensor], clear_frame: bool = False) -> None:
    """Append one agent's candidates after slot ``slot`` of ``buf.counts`` (slot 0 must hold 0).  ``clear_frame`` (round 6, ``coalign_anchor_decode_first``): this
    is the frame's first decode call -- its first launch zeroes ``buf.frame_words`` (what ``reset_frame`` did with a launch of its own)."""
    _need_gpu(cls, reg, anchors_f32)
    L = hip.lib()
    cls_c, reg_c = _f32c(cls), _f32c(reg)
    dir_c = None if dir_ is None else _f32c(dir_)
    if cls_c.dim() == 4:
        if cls_c.shape[0] != 1:
            raise ValueError("post-processing handles one frame at a time (batch size 1), like the reference")
        cls_c, reg_c = cls_c[0], reg_c[0]
        dir_c = None if dir_c is None else dir_c[0]
    A, H, W = cls_c.shape
    T = None if transform is None else _f32c(transform)
    args = (_ptr(cls_c), _ptr(reg_c), _ptr(dir_c), _ptr(anchors_f32), A, H, W, int(num_bins),
            float(score_thr), float(dir_offset), int(order == "hwl"), _ptr(T), buf.capacity,
            ctypes.c_void_p(buf.counts.data_ptr() + 4 * slot),
            ctypes.c_void_p(buf.counts.data_ptr() + 4 * (slot + 1)),
            _ptr(buf.cand_index), _ptr(buf.cand_score), _ptr(buf.cand_box7), _ptr(buf.cand_corners),
            _ptr(buf.cand_keep), _ptr(buf.status), _ptr(buf.dec_ws), buf.dec_ws_bytes)
    if clear_frame and _os.environ.get("COALIGN_PP_FILL") == "1":      # (measurement switch: the separate fill launch of rounds 2-5)
        buf.reset_frame()
        clear_frame = False
    if clear_frame:
        if slot != 0:
            raise ValueError("the frame's words are cleared by its FIRST decode call (slot 0)")
        hip.check(L.coalign_anchor_decode_first(*args, _ptr(buf.frame_words), buf.frame_words.numel(), _stream()), "coalign_anchor_decode_first")
    else:
        hip.check(L.coalign_anchor_decode(*args, _stream()), "coalign_anchor_decode")


@_device_op
def nms_rotated_device(boxes: torch.Tensor, scores: torch.Tensor, iou_thr: float, top: int = 1000,
                       valid: Optional[torch.Tensor] = None, k_dev: Optional[torch.Tensor] = None,
                       keep: Optional[torch.Tensor] = None, keep_count: Optional[torch.Tensor] = None,
                       ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """boxes [K, 8, 3] or [K, 4, 2] -> (keep int32 [top] device, keep_count int32 [1] device); no host sync."""
    _need_gpu(boxes, scores)
    L = hip.lib()
    b = _f32c(boxes)
    s = _f32c(scores)
    K = b.shape[0]
    rows, cols = (b.shape[1], b.shape[2]) if b.dim() == 3 else (4, 2)
    dev = b.device
    keep = torch.empty(top, dtype=torch.int32, device=dev) if keep is None else keep
    keep_count = torch.zeros(1, dtype=torch.int32, device=dev) if keep_count is None else keep_count
    ws_bytes = L.coalign_nms_rotated_workspace_bytes(K, top)
    if ws is None:
        ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device=dev)
    v = None if valid is None else valid.to(torch.uint8).contiguous()
    hip.check(L.coalign_nms_rotated(_ptr(b), rows, cols, _ptr(s), _ptr(v), K, _ptr(k_dev), float(iou_thr), top, _ptr(keep),
                                    _ptr(keep_count), _ptr(ws), ws.numel(), _stream()), "coalign_nms_rotated")
    return keep, keep_count


@_device_op
def nms_rotated_gather(corners: torch.Tensor, scores: torch.Tensor, iou_thr: float, top: int, valid: Optional[torch.Tensor], k_dev: Optional[torch.Tensor],
                       keep: torch.Tensor, keep_count: torch.Tensor, limit_range: Sequence[float], out_corners: torch.Tensor, out_scores: torch.Tensor,
                       out_count: torch.Tensor, ws: torch.Tensor) -> None:
    """``nms_rotated_device`` + ``gather_in_range`` as one C-ABI call (rank, bitmask, walk + gather: three launches); corners [K, 8, 3]."""
    _need_gpu(corners, scores, keep)
    L = hip.lib()
    b, s_ = _f32c(corners), _f32c(scores)
    if b.dim() != 3 or tuple(b.shape[1:]) != (8, 3):
        raise ValueError(f"corners must be [K, 8, 3], got {tuple(b.shape)}")
    v = None if valid is None else valid.to(torch.uint8).contiguous()
    r = (ctypes.c_double * 6)(*[float(x) for x in limit_range])
    hip.check(L.coalign_nms_rotated_gather(_ptr(b), _ptr(s_), _ptr(v), b.shape[0], _ptr(k_dev), float(iou_thr), int(top), _ptr(keep), _ptr(keep_count), r,
                                           _ptr(out_corners), _ptr(out_scores), _ptr(out_count), _ptr(ws), ws.numel(), _stream()), "coalign_nms_rotated_gather")


@_device_op
def gather_in_range(corners: torch.Tensor, scores: torch.Tensor, keep: torch.Tensor, keep_count: torch.Tensor,
                    limit_range: Sequence[float], out_corners: torch.Tensor, out_scores: torch.Tensor,
                    out_count: torch.Tensor) -> None:
    _need_gpu(corners, scores, keep)
    L = hip.lib()
    r = (ctypes.c_double * 6)(*[float(v) for v in limit_range])
    hip.check(L.coalign_gather_in_range(_ptr(corners), _ptr(scores), _ptr(keep), _ptr(keep_count), keep.numel(), r,
                                        _ptr(out_corners), _ptr(out_scores), _ptr(out_count), _stream()), "coalign_gather_in_range")


@_device_op
def iou_rotated_matrix(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """[Na, 8, 3] / [Na, 4, 2] corners x [Nb, ...] corners -> float32 IoU matrix [Na, Nb] (float64 clipping inside)."""
    _need_gpu(boxes_a, boxes_b)
    L = hip.lib()
    a, b = _f32c(boxes_a), _f32c(boxes_b)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if a.shape[0] and b.shape[0]:
        hip.check(L.coalign_iou_rotated_matrix(_ptr(a), a.shape[1], a.shape[2], a.shape[0], _ptr(b), b.shape[1], b.shape[2], b.shape[0],
                                               _ptr(out), _stream()), "coalign_iou_rotated_matrix")
    return out


@_device_op
def boxes_iou_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """OpenPCDet-semantics fp32 BEV IoU matrix [Na, Nb] of (x, y, z, dx, dy, dz, heading) boxes."""
    _need_gpu(boxes_a, boxes_b)
    L = hip.lib()
    a, b = _f32c(boxes_a), _f32c(boxes_b)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    hip.check(L.coalign_boxes_iou_bev(_ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out), _stream()), "coalign_boxes_iou_bev")
    return out


@_device_op
def bias_act_(y: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor] = None, relu: bool = True) -> torch.Tensor:
    """In place ``y = act(y + bias[c] (+ residual))`` on a contiguous NCHW float32 tensor (fused conv epilogue)."""
    _need_gpu(y, bias, residual)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("bias_act_ needs a contiguous float32 NCHW tensor")
    if residual is not None and (residual.shape != y.shape or not residual.is_contiguous() or residual.dtype != torch.float32):
        raise ValueError("residual must match y (contiguous float32)")
    N, C = y.shape[0], y.shape[1]
    HW = y.numel() // max(1, N * C)
    hip.check(hip.lib().coalign_bias_act(_ptr(y), _ptr(bias), _ptr(residual), N, C, HW, int(relu), _stream()), "coalign_bias_act")
    return y


VOX_FILTER_EGO, VOX_FILTER_RANGE = 1, 2   # COALIGN_VOX_FILTER_* of include/coalign_amd.h


@_device_op
def voxelize(points: torch.Tensor, cloud_offsets: Sequence[int], voxel_size: Sequence[float], lidar_range: Sequence[float],
             max_points: int, max_voxels: int, ego_filter: bool = False, filter_range: Optional[Sequence[float]] = None):
    """points [N, 4] (the clouds of a batch concatenated; ``cloud_offsets`` = host ints [n_clouds + 1]) ->
    (voxels [cap, max_points, 4], coords [cap, 4] int32 (cloud, z, y, x), num_points [cap] int32, counts [n_clouds + 1] int32).
    Only the first ``counts[-1]`` rows are meaningful; nothing here synchronises -- the caller slices after reading counts."""
    _need_gpu(points)
    L = hip.lib()
    pts = _f32c(points)
    if pts.dim() != 2 or pts.shape[1] != 4:
        raise ValueError(f"points must be [N, 4], got {tuple(pts.shape)}")
    n_clouds = len(cloud_offsets) - 1
    if int(cloud_offsets[-1]) != pts.shape[0]:
        raise ValueError("cloud_offsets[-1] must equal the number of points")
    off = (ctypes.c_int64 * (n_clouds + 1))(*[int(o) for o in cloud_offsets])
    vs, rg = _dbl3(voxel_size), (ctypes.c_double * 6)(*[float(v) for v in lidar_range])
    fr = None if filter_range is None else (ctypes.c_double * 6)(*[float(v) for v in filter_range])
    flags = (VOX_FILTER_EGO if ego_filter else 0) | (VOX_FILTER_RANGE if filter_range is not None else 0)
    cap = L.coalign_voxelize_capacity(pts.shape[0], n_clouds, vs, rg, int(max_voxels))
    if cap < 0:
        raise ValueError("invalid voxel grid / max_voxels")
    dev = pts.device
    voxels = torch.empty((cap, max_points, 4), dtype=torch.float32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty((cap,), dtype=torch.int32, device=dev)
    counts = torch.empty((n_clouds + 1,), dtype=torch.int32, device=dev)
    ws_bytes = L.coalign_voxelize_workspace_bytes(off, n_clouds, vs, rg, int(max_voxels))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    with _Timed("voxelize"):
        hip.check(L.coalign_voxelize(_ptr(pts), off, n_clouds, vs, rg, int(max_points), int(max_voxels), flags, fr, _ptr(voxels),
                                     _ptr(coords), _ptr(num), cap, _ptr(counts), _ptr(ws), ws_bytes, _stream()), "coalign_voxelize")
    return voxels, coords, num, counts


@_device_op
def pose_graph_optimize(vertex_offsets: torch.Tensor, edge_offsets: torch.Tensor, n_agents: torch.Tensor, vertices: torch.Tensor,
                        kinds: torch.Tensor, edge_agent: torch.Tensor, edge_landmark: torch.Tensor, edge_meas: torch.Tensor,
                        edge_info: torch.Tensor, max_iterations: int = 1000) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batched Levenberg-Marquardt over agent-object pose graphs (see include/coalign_amd.h (8)); all tensors on the device,
    offsets / indices int32, values float64.  -> (optimised vertices [V, 3], stats [G, 4])."""
    _need_gpu(vertex_offsets, edge_offsets, n_agents, vertices, kinds, edge_agent, edge_landmark, edge_meas, edge_info)
    L = hip.lib()
    i32 = lambda t: t.to(torch.int32).contiguous()
    f64 = lambda t: t.to(torch.float64).contiguous()
    vo, eo, na, kd, ea, el = (i32(t) for t in (vertex_offsets, edge_offsets, n_agents, kinds, edge_agent, edge_landmark))
    out, em, ew = f64(vertices).clone(), f64(edge_meas), f64(edge_info)
    G, V = na.shape[0], out.shape[0]
    stats = torch.zeros((G, 4), dtype=torch.float64, device=out.device)
    ws_bytes = L.coalign_pose_graph_workspace_bytes(V)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
    with _Timed("pose_graph_optimize"):
        hip.check(L.coalign_pose_graph_optimize(G, _ptr(vo), _ptr(eo), _ptr(na), V, _ptr(out), _ptr(kd), _ptr(ea), _ptr(el), _ptr(em), _ptr(ew),
                                                int(max_iterations), _ptr(stats), _ptr(ws), ws_bytes, _stream()), "coalign_pose_graph_optimize")
    return out, stats


# ---------------------------------------------------------------------------------------------- online pose correction (include/coalign_amd_align.h)
ALIGN_MAX_AGENTS, ALIGN_MAX_LANDMARKS = 8, 256
ALIGN_MAX_VERTICES = ALIGN_MAX_AGENTS + ALIGN_MAX_LANDMARKS
ALIGN_SOLVED, ALIGN_KEPT_NOISY, ALIGN_NO_BOXES, ALIGN_OUTSIDE_LIMITS, ALIGN_STORE_OVERFLOW, ALIGN_TOO_MANY_LANDMARKS = 0, 1, 2, 4, 8, 16
ALIGN_FLAG_BITS = {"use_uncertainty": 1, "landmark_SE2": 2, "adaptive_landmark": 4, "normalize_uncertainty": 8, "abandon_hard_cases": 16,
                   "drop_hard_boxes": 32, "drop_unsure_edge": 64}


class Stage1Store:
    """Caller-owned box store of ONE sample: the kept stage-1 detections of up to 8 agents, each in its agent's frame.  corners [8, C, 8, 3], uncertainty
    [8, C, udim], count [8] int32, status [1] int32 (``ALIGN_*``).  float32 is what ``stage1_gather`` fills; a float64 store takes boxes that did not come
    from the float32 stage-1 kernels (``upload``)."""

    def __init__(self, device, udim: int = 3, dtype: torch.dtype = torch.float32):
        if dtype not in (torch.float32, torch.float64) or not 0 <= int(udim) <= 3:
            raise ValueError("Stage1Store: float32 / float64, 0 <= udim <= 3")
        self.boxes = int(hip.lib().coalign_align_store_boxes())
        self.udim = int(udim)
        self.corners = torch.zeros((ALIGN_MAX_AGENTS, self.boxes, 8, 3), dtype=dtype, device=device)
        self.unc = torch.zeros((ALIGN_MAX_AGENTS, self.boxes, max(1, self.udim)), dtype=dtype, device=device)
        self.words = torch.zeros(ALIGN_MAX_AGENTS + 1, dtype=torch.int32, device=device)
        self.count, self.status = self.words[:ALIGN_MAX_AGENTS], self.words[ALIGN_MAX_AGENTS:]
        self.n_agents = 0

    def upload(self, corners_list, uncertainty_list=None) -> "Stage1Store":
        """Fill the store from host (or device) arrays, one [K_i, 8, 3] (and [K_i, udim]) per agent -- tests and tools; allocates and synchronises."""
        if len(corners_list) > ALIGN_MAX_AGENTS:
            raise ValueError(f"a sample has at most {ALIGN_MAX_AGENTS} agents")
        dev, dt = self.corners.device, self.corners.dtype
        words = [0] * (ALIGN_MAX_AGENTS + 1)
        for i, c in enumerate(corners_list):
            c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c).reshape(-1, 8, 3)
            n = min(int(c.shape[0]), self.boxes)
            words[i] = n
            if c.shape[0] > self.boxes:
                words[ALIGN_MAX_AGENTS] |= ALIGN_STORE_OVERFLOW
            self.corners[i, :n] = c[:n].to(device=dev, dtype=dt)
            if uncertainty_list is not None and self.udim:
                u = uncertainty_list[i]
                u = torch.as_tensor(np.asarray(u) if not torch.is_tensor(u) else u).reshape(-1, self.udim)
                self.unc[i, :n] = u[:n].to(device=dev, dtype=dt)
        self.words.copy_(torch.tensor(words, dtype=torch.int32))
        self.n_agents = len(corners_list)
        return self


@_device_op
def stage1_gather(buf: DecodeBuffers, unc: Optional[torch.Tensor], store: Stage1Store, slot: int) -> None:
    """After ``anchor_decode`` (slot 0, identity transform) + ``nms_rotated_device`` of ONE agent on ``buf``: copy the kept corners and the raw ``unc``
    ([A * udim, H, W]) of the kept anchors into slot ``slot`` of ``store``; slot 0 opens the frame's status word.  No host synchronisation."""
    _need_gpu(buf.counts, unc, store.corners)
    if store.corners.dtype != torch.float32:
        raise ValueError("stage1_gather fills a float32 store")
    A_udim, H, W = (0, 1, 1) if unc is None else unc.shape[-3:]
    A = buf.dec_A
    udim = 0 if unc is None else A_udim // A
    if udim != store.udim or (unc is not None and (A_udim % A or unc.dtype != torch.float32 or not unc.is_contiguous())):
        raise ValueError("unc must be contiguous float32 [A * udim, H, W] with the store's udim")
    if unc is None:
        H, W = buf.dec_HW
    hip.check(hip.lib().coalign_stage1_gather(_ptr(buf.keep), _ptr(buf.keep_count), _ptr(buf.cand_index), _ptr(buf.cand_corners), buf.capacity, _ptr(unc),
                                              A, udim, int(H), int(W), int(slot), _ptr(store.corners), _ptr(store.unc), _ptr(store.count), _ptr(store.status),
                                              _stream()), "coalign_stage1_gather")


def stage1_workspace(n_agents: int, A: int, H: int, W: int, top: int, device) -> torch.Tensor:
    """The workspace ``stage1_boxes`` needs for these head maps (include/coalign_amd_stage1.h (12a)); reused across frames by its owner."""
    n = int(hip.lib().coalign_stage1_boxes_workspace_bytes(int(n_agents), int(A), int(H), int(W), int(top)))
    if n == 0:
        raise ValueError(f"stage1_boxes: no workspace for {n_agents} agents, head maps {A} x {H} x {W}, top {top} (1 .. {ALIGN_MAX_AGENTS} agents, top <= 1024)")
    return torch.empty(n, dtype=torch.uint8, device=device)


@_device_op
def stage1_boxes(cls: torch.Tensor, reg: torch.Tensor, dir_: Optional[torch.Tensor], unc: Optional[torch.Tensor], anchors_f32: torch.Tensor, store: Stage1Store,
                 ws: torch.Tensor, score_thr: float, dir_offset: float, num_bins: int, order: str, iou_thr: float, top: int = 1000) -> None:
    """Stage 1 of ALL agents in one pass (``coalign_stage1_boxes``): the stage-1 model's head maps ``cls`` [n, A, H, W], ``reg`` [n, 7A, H, W], ``dir_``
    [n, bins * A, H, W] or None, ``unc`` [n, A * udim, H, W] or None -> slots 0 .. n - 1 of ``store`` and its status word, bit for bit what ``anchor_decode`` +
    ``nms_rotated_device`` + ``stage1_gather`` leave there agent by agent.  Five launches whatever n is, on the current stream; no host synchronisation."""
    _need_gpu(cls, reg, dir_, unc, anchors_f32, store.corners, ws)
    if store.corners.dtype != torch.float32:
        raise ValueError("stage1_boxes fills a float32 store")
    if cls.dim() != 4 or reg.dim() != 4:
        raise ValueError("stage1_boxes takes the head maps of a frame's agents: cls [n, A, H, W], reg [n, 7A, H, W]")
    def agent_dense(t):      # float32 with every agent's maps dense: read in place, agents t.stride(0) floats apart (channel slices of a merged-heads tensor)
        if t is None or (t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] >= 1 and t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel())):
            return t
        return _f32c(t)
    cls_c, reg_c, dir_c, unc_c = agent_dense(cls), agent_dense(reg), agent_dense(dir_), agent_dense(unc)
    n, A, H, W = cls_c.shape
    udim = 0 if unc_c is None else unc_c.shape[1] // A
    if tuple(reg_c.shape) != (n, 7 * A, H, W) or (dir_c is not None and tuple(dir_c.shape) != (n, int(num_bins) * A, H, W)):
        raise ValueError("stage1_boxes: reg [n, 7A, H, W] and dir [n, num_bins * A, H, W] must match cls [n, A, H, W]")
    if udim != store.udim or (unc_c is not None and tuple(unc_c.shape) != (n, A * udim, H, W)):
        raise ValueError("unc must be [n, A * udim, H, W] with the store's udim")
    if anchors_f32.dtype != torch.float32 or not anchors_f32.is_contiguous() or anchors_f32.numel() != A * H * W * 7:
        raise ValueError("anchors: contiguous float32 [H * W * A, 7]")
    stride = lambda t: 0 if t is None else (int(t.stride(0)) if n > 1 else int(t[0].numel()))      # (one agent: its stride is never used and may be anything)
    hip.check(hip.lib().coalign_stage1_boxes_strided(_ptr(cls_c), _ptr(reg_c), _ptr(dir_c), _ptr(unc_c if udim else None), stride(cls_c), stride(reg_c), stride(dir_c),
                                                     stride(unc_c), _ptr(anchors_f32), n, A, H, W, int(num_bins), udim, float(score_thr), float(dir_offset),
                                                     int(order == "hwl"), float(iou_thr), int(top), _ptr(store.corners), _ptr(store.unc), _ptr(store.count),
                                                     _ptr(store.status), _ptr(ws), ws.numel(), _stream()), "coalign_stage1_boxes_strided")


class PoseGraphArrays:
    """The graph arrays of one sample at their fixed capacities (what ``coalign_pose_graph_optimize`` reads for one graph), the solver's workspace and stats."""

    def __init__(self, device):
        L = hip.lib()
        V, E = ALIGN_MAX_VERTICES, ALIGN_MAX_AGENTS * int(L.coalign_align_store_boxes())
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)
        self.vertex_off, self.edge_off, self.n_agents = i32(2), i32(2), i32(1)
        self.vertices, self.kinds = f64(V, 3), i32(V)
        self.edge_agent, self.edge_landmark, self.edge_meas, self.edge_info = i32(E), i32(E), f64(E, 3), f64(E, 3)
        self.stats = f64(1, 4)
        self.ws_bytes = L.coalign_pose_graph_workspace_bytes(V)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)


def align_flags(**flags) -> int:
    """Keyword arguments of ``box_alignment_relative_sample_np`` -> the flag word of ``coalign_pose_graph_build`` (the reference's defaults)."""
    given = dict({"use_uncertainty": True, "landmark_SE2": True}, **flags)
    unknown = set(given) - set(ALIGN_FLAG_BITS)
    if unknown:
        raise ValueError(f"unknown box alignment flags {sorted(unknown)}")
    return sum(bit for name, bit in ALIGN_FLAG_BITS.items() if given.get(name, False))


@_device_op
def pose_graph_build(store: Stage1Store, noisy_poses: torch.Tensor, graph: PoseGraphArrays, flags: int, thres: float = 1.5, yaw_var_thres: float = 0.2,
                     with_uncertainty: bool = True) -> None:
    """``box_align.build_pose_graph`` on the device: ``store`` + noisy poses [N, 6] float64 (degrees) -> ``graph`` and the sample's status word
    (``store.status``).  One launch, no host synchronisation."""
    _need_gpu(store.corners, noisy_poses, graph.vertices)
    if noisy_poses.dtype != torch.float64 or noisy_poses.dim() != 2 or noisy_poses.shape[1] != 6 or not noisy_poses.is_contiguous():
        raise ValueError("noisy_poses must be contiguous float64 [N, 6]")
    unc = store.unc if (with_uncertainty and store.udim) else None
    hip.check(hip.lib().coalign_pose_graph_build(1, int(noisy_poses.shape[0]), _ptr(store.corners), _ptr(unc), int(store.corners.dtype == torch.float64), store.udim,
                                                 _ptr(store.count), _ptr(noisy_poses), int(flags), float(thres), float(yaw_var_thres), _ptr(graph.vertex_off),
                                                 _ptr(graph.edge_off), _ptr(graph.n_agents), _ptr(graph.vertices), _ptr(graph.kinds), _ptr(graph.edge_agent),
                                                 _ptr(graph.edge_landmark), _ptr(graph.edge_meas), _ptr(graph.edge_info), _ptr(store.status), _stream()),
              "coalign_pose_graph_build")


@_device_op
def pose_graph_solve(graph: PoseGraphArrays, max_iterations: int = 1000) -> None:
    """``coalign_pose_graph_optimize`` in place on the arrays ``pose_graph_build`` wrote (offsets read on the device; the capacity as ``total_vertices``)."""
    _need_gpu(graph.vertices)
    hip.check(hip.lib().coalign_pose_graph_optimize(1, _ptr(graph.vertex_off), _ptr(graph.edge_off), _ptr(graph.n_agents), ALIGN_MAX_VERTICES, _ptr(graph.vertices),
                                                    _ptr(graph.kinds), _ptr(graph.edge_agent), _ptr(graph.edge_landmark), _ptr(graph.edge_meas), _ptr(graph.edge_info),
                                                    int(max_iterations), _ptr(graph.stats), _ptr(graph.ws), graph.ws_bytes, _stream()), "coalign_pose_graph_optimize")


@_device_op
def pose_correct_matrices(noisy_poses: torch.Tensor, vertices: torch.Tensor, status: torch.Tensor, max_cav: int, H: int, W: int, den_x: float, den_y: float,
                          proj_first: bool, poses_out: torch.Tensor, pairwise: torch.Tensor, affine: torch.Tensor) -> None:
    """Refined (x, y, yaw) (or the noisy poses, by ``status``) -> corrected poses [N, 6], pairwise [1, L, L, 4, 4], normalised affine [1, L, L, 2, 3], float64."""
    _need_gpu(noisy_poses, vertices, status, poses_out, pairwise, affine)
    n = int(noisy_poses.shape[0])
    ok = (noisy_poses.dtype == torch.float64 and noisy_poses.is_contiguous() and tuple(noisy_poses.shape) == (n, 6) and vertices.dtype == torch.float64
          and tuple(vertices.shape) == (ALIGN_MAX_VERTICES, 3) and vertices.is_contiguous() and status.dtype == torch.int32
          and poses_out.dtype == torch.float64 and tuple(poses_out.shape) == (n, 6) and poses_out.is_contiguous()
          and pairwise.dtype == torch.float64 and pairwise.numel() == max_cav * max_cav * 16 and pairwise.is_contiguous()
          and affine.dtype == torch.float64 and affine.numel() == max_cav * max_cav * 6 and affine.is_contiguous())
    if not ok:
        raise ValueError("pose_correct_matrices: float64 contiguous [N, 6] poses, [264, 3] vertices, [L, L, 4, 4] / [L, L, 2, 3] outputs, int32 status")
    hip.check(hip.lib().coalign_pose_correct_matrices(1, n, _ptr(noisy_poses), _ptr(vertices), _ptr(status), int(max_cav), int(bool(proj_first)), int(H), int(W),
                                                      float(den_x), float(den_y), _ptr(poses_out), _ptr(pairwise), _ptr(affine), _stream()),
              "coalign_pose_correct_matrices")


CONV_KC, CONV_WSTRIDE = 8, 9 * 64 + 32      # kKC / kWStride of csrc/conv3x3.hip
_CONV_WS: dict = {}
_CONV_WS_RETIRED: list = []      # outgrown workspaces stay allocated: HIP graphs captured earlier on the lane still hold their raw pointers.  Bounded: a
                                 # workspace only grows when a LARGER shape arrives on its stream, i.e. at most once per distinct layer shape and stream.


def _conv_workspace(key, ws_bytes: int, device) -> torch.Tensor:
    """One stream-K workspace per (device, stream[, kernel family]): launches on a stream are ordered.  A workspace that has to grow is
    replaced, never freed (a captured graph replays with the pointer it was captured with; flags and partials of different launches on one
    stream never overlap in time, so the retired buffer stays private to those graphs)."""
    ws = _CONV_WS.get(key)
    if ws is None or ws.numel() < ws_bytes:
        if ws is not None:
            _CONV_WS_RETIRED.append(ws)
        ws = _CONV_WS[key] = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    return ws


def pack_conv3x3_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [Cout / 64, Cin / 8, 8, 608]: per 64-channel group and 8-input-channel chunk the exact LDS image
    coalign_conv3x3_bias_act streams in ([ci][tap][64 couts] + 32 zero floats of bank padding per input channel)."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or co % 64 or ci % CONV_KC:
        raise ValueError(f"conv3x3 kernel needs 3x3 weights with Cout % 64 == 0 and Cin % 8 == 0, got {tuple(weight.shape)}")
    w = weight.detach().float().reshape(co // 64, 64, ci // CONV_KC, CONV_KC, 9).permute(0, 2, 3, 4, 1)   # [g, chunk, k, tap, 64]
    out = torch.zeros((co // 64, ci // CONV_KC, CONV_KC, CONV_WSTRIDE), dtype=torch.float32, device=weight.device)
    out[..., : 9 * 64] = w.reshape(co // 64, ci // CONV_KC, CONV_KC, 9 * 64)
    return out.contiguous()


@_device_op
def conv3x3_bias_act(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor] = None,
                     relu: bool = True) -> torch.Tensor:
    """y = act(conv3x3(x, w) + bias (+ residual)), stride 1, padding 1, NCHW float32, on the fp32 matrix cores."""
    _need_gpu(x, w_packed, bias, residual)
    L = hip.lib()
    xc = _f32c(x)
    N, Cin, H, W = xc.shape
    G, n_chunks, _, _ = w_packed.shape
    Cin_w = n_chunks * CONV_KC
    if Cin_w != Cin:
        raise ValueError(f"input has {Cin} channels, packed weight expects {Cin_w}")
    Cout = G * 64
    y = torch.empty((N, Cout, H, W), dtype=torch.float32, device=xc.device)
    res = None if residual is None else _f32c(residual)
    if res is not None and res.shape != y.shape:
        raise ValueError("residual shape mismatch")
    ws_bytes = L.coalign_conv3x3_workspace_bytes(N, Cin, Cout, H, W)
    key = (xc.device, torch.cuda.current_stream(xc.device).cuda_stream)
    ws = _conv_workspace(key, ws_bytes, xc.device)
    b = torch.zeros(Cout, dtype=torch.float32, device=xc.device) if bias is None else _f32c(bias)
    with _Timed("conv3x3_bias_act"):
        hip.check(L.coalign_conv3x3_bias_act(_ptr(xc), _ptr(w_packed), _ptr(b), _ptr(res), _ptr(y),
                                             N, Cin, Cout, H, W, int(relu), _ptr(ws), ws.numel(), _stream()), "coalign_conv3x3_bias_act")
    return y


def pack_conv3x3_emu_weight(weight: torch.Tensor, terms: int = 3, tap_major: bool = False) -> torch.Tensor:
    """[Cout, Cin, 3, 3] fp32 -> the split-bf16 LDS image of csrc/conv3x3_emu.hip, as uint8:
    [Cout / 64][Cin / 8][5 steps][terms][2 k-groups][64 cout][8 cin] bf16 (tap = 2 * step + k-group, the tenth tap is zero;
    term 0 = bf16(w), term 1 = bf16(w - term 0), term 2 = bf16(w - term 0 - term 1)) followed by 16 zero bytes; ``terms`` = 16: two fp16 terms of the
    per-channel scaled weights (below) followed by 16 zero bytes, [Cout] float32 2^-k_c and [Cout] float32 2^k_c.
    ``tap_major`` (Cin % 16 == 0): [Cout / 64][Cin / 16][9 taps][terms][2 channel halves][64 cout][8 cin] -- one matrix
    instruction = the 16 channels of one tap, no zero tap (COALIGN_LAYOUT_W_TAPMAJOR)."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or co % 64 or ci % (2 * CONV_KC if tap_major else CONV_KC) or terms not in (2, 3, 16):
        raise ValueError(f"conv3x3_emu needs 3x3 weights with Cout % 64 == 0, Cin % 8 == 0 (16 tap-major) and terms in (2, 3, 16), got {tuple(weight.shape)}, {terms}")
    if tap_major:
        w = weight.detach().float().reshape(co // 64, 64, ci // (2 * CONV_KC), 2, CONV_KC, 9)
        w = w.permute(0, 2, 5, 3, 1, 4)                                    # [g, interval, tap, channel half, cout, cin]
    else:
        w = weight.detach().float().reshape(co // 64, 64, ci // CONV_KC, CONV_KC, 9)
        w = torch.cat([w, torch.zeros_like(w[..., :1])], dim=-1).reshape(co // 64, 64, ci // CONV_KC, CONV_KC, 5, 2)
        w = w.permute(0, 2, 4, 5, 1, 3)                                    # [g, chunk, step, k-group, cout, cin]
    tail = []
    if terms == 16:
        # fp16 split = sp16 pairs (csrc/common.h).  Every output channel is first multiplied by the power of two 2^k_c that puts its largest weight into
        # [2^13, 2^14) (exact), so that both terms are normal fp16 numbers whatever the channel's scale (BatchNorm-folded weights are mostly below 2^-3, where
        # an unscaled second term is an fp16 subnormal); the kernel multiplies bias + residual by 2^k_c and the finished tile by 2^-k_c (both exact).
        # w~ = w 2^k_c rounded to 22 significant bits; term 0 = fp16(w~) to nearest, term 1 = (w~ - term 0) * 2^10, exact.
        amax = weight.detach().float().abs().reshape(co, -1).amax(dim=1)
        k = torch.where(amax > 0, 14 - torch.frexp(amax)[1], torch.zeros_like(amax, dtype=torch.int32)).clamp(-60, 60).to(torch.int32)
        scale = torch.ldexp(torch.ones_like(amax), k)
        cshape = (co // 64, 1, 1, 1, 64, 1)                                # the output channel sits on axis 4 of both images
        ws = (w * scale.reshape(cshape)).contiguous()
        ws = ((ws.view(torch.int32) + 2) & -4).view(torch.float32)         # 22 significant bits, ties away from zero (sp16_round)
        hi = ws.half()
        lo = ((ws - hi.float()) * 1024.0).half()
        parts = [hi, lo]
        tail = [torch.ldexp(torch.ones_like(amax), -k).contiguous().view(torch.uint8).reshape(-1), scale.contiguous().view(torch.uint8).reshape(-1)]
    else:
        parts, rest = [], w
        for _ in range(terms):
            t = rest.bfloat16()
            parts.append(t)
            rest = rest - t.float()
    img = torch.stack(parts, dim=3).contiguous()                           # [g, chunk, step, term, k-group, cout, cin]
    flat = img.view(torch.uint8).reshape(-1)
    out = torch.cat([flat, torch.zeros(16, dtype=torch.uint8, device=flat.device)] + tail)
    assert out.numel() == hip.lib().coalign_conv3x3_emu_weight_bytes_ex(ci, co, terms, int(tap_major))
    return out


LAYOUT_NCHW, LAYOUT_OUT_NHWC, LAYOUT_IN_NHWC, LAYOUT_W_TAPMAJOR, LAYOUT_OUT_SP = 0, 1, 2, 4, 8      # COALIGN_LAYOUT_* of include/coalign_amd.h


def is_channels_last(t: torch.Tensor) -> bool:
    """A 4-d tensor whose memory order is (N, H, W, C) and not at the same time plain NCHW (C > 1, H * W > 1)."""
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


@_device_op
def conv3x3_emu_bias_act(x: torch.Tensor, w_split: torch.Tensor, bias: torch.Tensor, cout: int, residual: Optional[torch.Tensor] = None,
                         relu: bool = True, terms: int = 3, stride: int = 1, out_channels_last: bool = False, out_split: bool = False):
    """y = act(conv3x3(x, w, stride, padding 1) + bias (+ residual)) with every fp32 product evaluated from 16-bit terms on the matrix cores, fp32 accumulation
    (csrc/conv3x3_emu.hip): ``terms`` = 16 -- the detector's default arithmetic -- sp16 pairs on the fp16 cores (22-bit operands, scale free), 3 / 2 = 3- / 2-way
    bf16 split (the signature's default of 3 dates from rounds 2-3; the detector passes ``backbone.CONV_EMU_TERMS``).  A channels-last ``x`` is read in place by the
    stride-2 variant; ``out_channels_last`` (stride 1) returns a tensor of logical shape [N, C, H, W] in channels-last memory; ``out_split`` (terms 16, no
    residual: the strided layers and the tap-major stride-1 image on an NCHW input) returns a ``SplitMap``."""
    _need_gpu(x, w_split, bias, residual)
    L = hip.lib()
    layout = LAYOUT_NCHW
    if x.dtype == torch.float32 and stride == 2 and is_channels_last(x):
        xc, layout = x, LAYOUT_IN_NHWC
    else:
        xc = _f32c(x)
    N, Cin, H, W = xc.shape
    tapk = 0                                               # the two weight images differ in size (9 : 10): recognised by it
    if w_split.numel() != L.coalign_conv3x3_emu_weight_bytes(Cin, cout, terms):
        if stride != 1 or w_split.numel() != L.coalign_conv3x3_emu_weight_bytes_ex(Cin, cout, terms, 1):
            raise ValueError("split weight image does not match (Cin, Cout, terms)")
        tapk = LAYOUT_W_TAPMAJOR
    if stride not in (1, 2) or (stride == 2 and (residual is not None or (out_channels_last and layout != LAYOUT_IN_NHWC))):
        raise ValueError("stride 2 takes no residual and writes NCHW (channels-last only from a channels-last input)")
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    out = None
    if out_split:
        if terms != 16 or residual is not None or out_channels_last or (stride == 1 and (not tapk or layout != LAYOUT_NCHW)):
            raise ValueError("SplitMap output: terms 16, no residual; stride 2, or stride 1 with the tap-major image on an NCHW input")
        layout |= LAYOUT_OUT_SP
        out = SplitMap.empty(N, cout, Ho, Wo, xc.device)
        y = out.data
    elif out_channels_last:
        layout |= LAYOUT_OUT_NHWC
        y = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=xc.device, memory_format=torch.channels_last)
    else:
        y = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=xc.device)
    res = None if residual is None else _f32c(residual)
    if res is not None and res.shape != y.shape:
        raise ValueError("residual shape mismatch")
    ws, ws_bytes = None, 0
    layout |= tapk
    if stride == 1 and (layout & 3) == LAYOUT_NCHW:
        ws_bytes = L.coalign_conv3x3_emu_workspace_bytes_ex(N, Cin, cout, H, W, terms, layout)
    if ws_bytes:
        key = (xc.device, torch.cuda.current_stream(xc.device).cuda_stream, "emu")
        ws = _conv_workspace(key, ws_bytes, xc.device)
    with _Timed("conv3x3_emu_bias_act"):
        hip.check(L.coalign_conv3x3_emu_ex(_ptr(xc), _ptr(w_split), _ptr(_f32c(bias)), _ptr(res), _ptr(y), N, Cin, cout, H, W, int(stride),
                                           int(relu), terms, layout, _ptr(sp_range_flag(xc.device)) if out_split else None, _ptr(ws), 0 if ws is None else ws.numel(), _stream()),
                  "coalign_conv3x3_emu_ex")
    return y if out is None else out


_SP_WS: dict = {}
_SP_WS_RETIRED: list = []
SP_WS_MIN_BYTES = 24 << 20          # the largest stream-K workspace of the shipped configs (256 workgroups x 8 wavefronts x 8 KB + flags) is 16.8 MB


def _sp_workspace(device, ws_bytes: int) -> torch.Tensor:
    """The stream-K workspace of ``coalign_conv3x3_sp`` for the CURRENT stream of ``device``: zero-initialised once (the launches leave their flag words zero
    again), one per stream (launches on a stream are ordered), sized for every shipped shape on first use so that it never grows inside a captured frame; a
    workspace that still has to grow is replaced and kept referenced (captured graphs hold its pointer)."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _SP_WS.get(key)
    if ws is None or ws.numel() < ws_bytes:
        if ws is not None:
            _SP_WS_RETIRED.append(ws)
        ws = _SP_WS[key] = torch.zeros(max(ws_bytes, SP_WS_MIN_BYTES), dtype=torch.uint8, device=device)
    return ws


# Measurement switch (round 6): COALIGN_SP_GEO="25x88:121,50x176:81" overrides the tile geometry `coalign_conv3x3_sp` picks for maps of the listed H x W
# (codes: include/coalign_amd.h (9e)); read once at import, the dict is read per call.
SP_GEO_OVERRIDE = {tuple(int(v) for v in k.split("x")): int(g) for k, g in (item.split(":") for item in _os.environ.get("COALIGN_SP_GEO", "").split(",") if item)}

SP_RES_NONE, SP_RES_SP, SP_RES_NHWC = 0, 1, 2      # residual_kind of coalign_conv3x3_sp
SP_OUT_SP, SP_OUT_NHWC = 1, 2                      # out_kind


@_device_op
def conv3x3_sp(x: "SplitMap", w_split: torch.Tensor, bias: torch.Tensor, cout: int, residual=None, relu: bool = True, out_split: bool = True, geometry: int = 0,
               out_both: bool = False):
    """y = act(conv3x3(x, w, stride 1, padding 1) + bias (+ residual)) on a ``SplitMap`` input (include/coalign_amd.h (9e), csrc/conv3x3_sp.hip): the fp16
    mode's arithmetic with the operand split done by the producer.  ``w_split``: the tap-major terms-16 image of ``pack_conv3x3_emu_weight``; ``residual``: a
    SplitMap, a float32 tensor (converted to channels-last memory if it is not) or None; returns a SplitMap (``out_split``) or a float32 tensor of logical
    shape [N, C, H, W] in channels-last memory; ``out_both`` (round 6, ``coalign_conv3x3_sp_both``): the pair (channels-last float32 tensor, SplitMap of it)."""
    if not isinstance(x, SplitMap):
        raise TypeError("conv3x3_sp reads a SplitMap")
    if out_both:
        out_split = False
    _need_gpu(x.data, w_split, bias)
    L = hip.lib()
    N, Cin, H, W = x.shape
    if geometry == 0 and SP_GEO_OVERRIDE:
        geometry = SP_GEO_OVERRIDE.get((H, W), 0)
    if w_split.numel() != L.coalign_conv3x3_emu_weight_bytes_ex(Cin, cout, 16, 1):
        raise ValueError("conv3x3_sp needs the tap-major terms-16 weight image of (Cin, Cout)")
    res_kind, res_t = SP_RES_NONE, None
    if isinstance(residual, SplitMap):
        res_kind, res_t = SP_RES_SP, residual.data
        if residual.shape != (N, cout, H, W):
            raise ValueError("residual shape mismatch")
    elif residual is not None:
        res_kind, res_t = SP_RES_NHWC, to_nhwc(residual)
        if tuple(res_t.shape) != (N, cout, H, W):
            raise ValueError("residual shape mismatch")
    if out_split:
        out = SplitMap.empty(N, cout, H, W, x.device)
        y = out.data
    else:
        out = y = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        if not nhwc_memory(y):
            out = y = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
    ws_bytes = L.coalign_conv3x3_sp_workspace_bytes(N, Cin, cout, H, W, int(geometry))
    ws = _sp_workspace(x.device, ws_bytes) if ws_bytes else None
    if out_both:
        both = SplitMap.empty(N, cout, H, W, x.device)
        with _Timed("conv3x3_sp"):
            hip.check(L.coalign_conv3x3_sp_both(_ptr(x.data), _ptr(w_split), _ptr(_f32c(bias)), _ptr(res_t), res_kind, _ptr(y), _ptr(both.data), N, Cin, cout, H, W, int(relu), int(geometry),
                                                _ptr(sp_range_flag(x.device)), _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "coalign_conv3x3_sp_both")
        return out, both
    with _Timed("conv3x3_sp"):
        hip.check(L.coalign_conv3x3_sp(_ptr(x.data), _ptr(w_split), _ptr(_f32c(bias)), _ptr(res_t), res_kind, _ptr(y), SP_OUT_SP if out_split else SP_OUT_NHWC,
                                       N, Cin, cout, H, W, int(relu), int(geometry), _ptr(sp_range_flag(x.device)) if out_split else None,
                                       _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "coalign_conv3x3_sp")
    return out


NARROW_COUTS = (16, 32)                            # output widths of coalign_conv3x3_sp_narrow (include/coalign_amd_narrow.h)
NARROW_IN_SP, NARROW_IN_NHWC = 0, 1                # in_kind


def pack_conv3x3_narrow_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] fp32 (Cout 16 or 32, Cin % 16 == 0) -> the weight image of ``coalign_conv3x3_sp_narrow`` as uint8 (include/coalign_amd_narrow.h):
    [Cin / 16][9 taps][2 terms][2 channel halves][Cout][8 cin] fp16 sp16 pairs of the per-output-channel scaled weights (the scaling and rounding of
    ``pack_conv3x3_emu_weight``'s terms-16 image: the two images hold the same pairs), 16 zero bytes, [Cout] float32 2^-k_c, [Cout] float32 2^k_c."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or co not in NARROW_COUTS or ci % 16 or ci < 16:
        raise ValueError(f"conv3x3_sp_narrow needs 3x3 weights with Cout in {NARROW_COUTS} and Cin % 16 == 0, got {tuple(weight.shape)}")
    wf = weight.detach().float()
    w = wf.reshape(co, ci // 16, 2, 8, 9).permute(1, 4, 2, 0, 3)          # [interval, tap, channel half, cout, cin]
    amax = wf.abs().reshape(co, -1).amax(dim=1)
    k = torch.where(amax > 0, 14 - torch.frexp(amax)[1], torch.zeros_like(amax, dtype=torch.int32)).clamp(-60, 60).to(torch.int32)
    scale = torch.ldexp(torch.ones_like(amax), k)
    ws = (w * scale.reshape(1, 1, 1, co, 1)).contiguous()
    ws = ((ws.view(torch.int32) + 2) & -4).view(torch.float32)             # 22 significant bits, ties away from zero (sp16_round)
    hi = ws.half()
    lo = ((ws - hi.float()) * 1024.0).half()
    flat = torch.stack([hi, lo], dim=2).contiguous().view(torch.uint8).reshape(-1)      # [interval, tap, term, channel half, cout, cin]
    tail = [torch.ldexp(torch.ones_like(amax), -k).contiguous().view(torch.uint8).reshape(-1), scale.contiguous().view(torch.uint8).reshape(-1)]
    out = torch.cat([flat, torch.zeros(16, dtype=torch.uint8, device=flat.device)] + tail)
    assert out.numel() == hip.lib().coalign_conv3x3_narrow_weight_bytes(ci, co)
    return out


@_device_op
def conv3x3_sp_narrow(x, w_narrow: torch.Tensor, bias: torch.Tensor, cout: int, relu: bool = True) -> "SplitMap":
    """y = act(conv3x3(x, w, stride 1, padding 1) + bias) with 16 or 32 output channels, written as a ``SplitMap`` (include/coalign_amd_narrow.h,
    csrc/conv3x3_narrow.hip: NaiveCompressor's encoder).  ``x``: a SplitMap, or a float32 tensor of logical shape [N, C, H, W] -- read in place when its
    memory is channels-last (the kernel's loader splits it), packed with ``SplitMap.pack`` first when it is NCHW -- or a ``SparseCanvas`` (Cin >= 32), whose rows
    are packed to sp16 rows and gathered through its stamps (include/coalign_amd_narrow_sparse.h): no dense canvas exists.  ``w_narrow``: ``pack_conv3x3_narrow_weight``."""
    if isinstance(x, SparseCanvas):
        x.check_current()
        L = hip.lib()
        N, Cin, H, W = x.shape
        _need_gpu(w_narrow, bias)
        if cout not in NARROW_COUTS or Cin % 16 or w_narrow.numel() != L.coalign_conv3x3_narrow_weight_bytes(Cin, cout):
            raise ValueError("conv3x3_sp_narrow needs the narrow weight image of (Cin, Cout), Cout 16 or 32, Cin % 16 == 0")
        rows = sp_pack_rows(x)
        out = SplitMap.empty(N, cout, H, W, x.device)
        with _Timed("conv3x3_sp_narrow_sparse"):
            hip.check(L.coalign_conv3x3_sp_narrow_sparse(_rows_ptr(rows), int(rows.shape[0]), _ptr(x.stamps), _ptr(x.state), _ptr(w_narrow), _ptr(_f32c(bias)), _ptr(out.data),
                                                         N, Cin, cout, H, W, int(relu), _ptr(sp_range_flag(x.device)), _stream()), "coalign_conv3x3_sp_narrow_sparse")
        return out
    if isinstance(x, SplitMap):
        kind, xt = NARROW_IN_SP, x.data
        N, Cin, H, W = x.shape
    else:
        _need_gpu(x)
        if x.dim() != 4:
            raise ValueError("conv3x3_sp_narrow reads a SplitMap or a [N, C, H, W] tensor")
        N, Cin, H, W = x.shape
        if nhwc_memory(x):
            kind, xt = NARROW_IN_NHWC, x
        else:
            x = SplitMap.pack(x)
            kind, xt = NARROW_IN_SP, x.data
    _need_gpu(xt, w_narrow, bias)
    L = hip.lib()
    if cout not in NARROW_COUTS or Cin % 16 or w_narrow.numel() != L.coalign_conv3x3_narrow_weight_bytes(Cin, cout):
        raise ValueError("conv3x3_sp_narrow needs the narrow weight image of (Cin, Cout), Cout 16 or 32, Cin % 16 == 0")
    out = SplitMap.empty(N, cout, H, W, xt.device)
    with _Timed("conv3x3_sp_narrow"):
        hip.check(L.coalign_conv3x3_sp_narrow(_ptr(xt), kind, _ptr(w_narrow), _ptr(_f32c(bias)), _ptr(out.data), N, Cin, cout, H, W, int(relu),
                                              _ptr(sp_range_flag(xt.device)), _stream()), "coalign_conv3x3_sp_narrow")
    return out


@_device_op
def sp_pack_rows(sc: "SparseCanvas") -> torch.Tensor:
    """The feature rows of a ``SparseCanvas`` as sp16 rows [M, C / 16, 4, 8] float16 (``coalign_sp_pack_rows``, include/coalign_amd.h (9f)): what the LDS-DMA
    gather of ``conv3x3_sp_s2`` reads.  Rows at and beyond the device-side count (if the canvas has one) are left untouched."""
    L = hip.lib()
    M, C = int(sc.feats.shape[0]), sc.C
    out = torch.empty((max(M, 1), C // 16, 4, 8), dtype=torch.float16, device=sc.device)[:M]
    with _Timed("sp_pack_rows"):
        hip.check(L.coalign_sp_pack_rows(_rows_ptr(sc.feats), M, _ptr(sc.count_dev) if sc.count_dev is not None else _ptr(getattr(sc, "count_word", None)), C, _rows_ptr(out),
                                         _ptr(sp_range_flag(sc.device)), _stream()), "coalign_sp_pack_rows")
    return out


def pack_conv1x1_sp_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin] (or [Cout, Cin, 1, 1]) fp32 -> the sp16 image of the 1 x 1 skip convolution that rides in ``conv3x3_sp_s2`` (include/coalign_amd.h (9g)): the
    centre-tap slice of the tap-major terms-16 image of ``pack_conv3x3_emu_weight`` (same per-output-channel scale rule), as uint8."""
    w = weight.detach().float().reshape(weight.shape[0], weight.shape[1])
    co, ci = w.shape
    w3 = torch.zeros((co, ci, 3, 3), dtype=torch.float32, device=w.device)
    w3[:, :, 1, 1] = w
    img = pack_conv3x3_emu_weight(w3, 16, True)
    body = co * ci * 9 * 4                                    # two fp16 terms per weight
    taps = img[:body].view(torch.float16).reshape(co // 64, ci // 16, 9, 2 * 2 * 64 * 8)
    out = torch.cat([taps[:, :, 4].contiguous().view(torch.uint8).reshape(-1), img[body:]])
    assert out.numel() == hip.lib().coalign_conv1x1_sp_weight_bytes(ci, co)
    return out


@_device_op
def conv3x3_sp_s2(x, w_split: torch.Tensor, bias: torch.Tensor, cout: int, relu: bool = True, w_skip: Optional[torch.Tensor] = None):
    """y = act(conv3x3(x, w, stride 2, padding 1) + bias) on split operands (include/coalign_amd.h (9f), csrc/conv3x3_sp_s2.hip): ``x`` a ``SplitMap`` or a
    ``SparseCanvas`` (its rows are packed to sp16 rows first); ``w_split``: the tap-major terms-16 image of ``pack_conv3x3_emu_weight``; returns a ``SplitMap``.
    ``w_skip`` (``pack_conv1x1_sp_weight``; (9g)): the block's 1 x 1 / stride-2 skip convolution rides along as a tenth tap -- returns (SplitMap, skip map: float32
    of logical shape [N, Cout, Ho, Wo] in channels-last memory, no bias, no ReLU)."""
    L = hip.lib()
    N, Cin, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if w_split.numel() != L.coalign_conv3x3_emu_weight_bytes_ex(Cin, cout, 16, 1):
        raise ValueError("conv3x3_sp_s2 needs the tap-major terms-16 weight image of (Cin, Cout)")
    if w_skip is not None and w_skip.numel() != L.coalign_conv1x1_sp_weight_bytes(Cin, cout):
        raise ValueError("conv3x3_sp_s2: the skip image does not match (Cin, Cout)")
    out = SplitMap.empty(N, cout, Ho, Wo, x.device)
    skip = None if w_skip is None else torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
    flag = _ptr(sp_range_flag(x.device))
    b = _f32c(bias)
    if isinstance(x, SparseCanvas):
        x.check_current()
        rows = sp_pack_rows(x)
        with _Timed("conv3x3_sp_s2_sparse"):
            if w_skip is None:
                hip.check(L.coalign_conv3x3_sp_s2_sparse(_rows_ptr(rows), int(rows.shape[0]), _ptr(x.stamps), _ptr(x.state), _ptr(w_split), _ptr(b), _ptr(out.data),
                                                         N, Cin, cout, H, W, int(relu), flag, _stream()), "coalign_conv3x3_sp_s2_sparse")
            else:
                hip.check(L.coalign_conv3x3_sp_s2_skip_sparse(_rows_ptr(rows), int(rows.shape[0]), _ptr(x.stamps), _ptr(x.state), _ptr(w_split), _ptr(b), _ptr(w_skip), _ptr(out.data),
                                                              _ptr(skip), N, Cin, cout, H, W, int(relu), flag, _stream()), "coalign_conv3x3_sp_s2_skip_sparse")
        return out if w_skip is None else (out, skip)
    if not isinstance(x, SplitMap):
        raise TypeError("conv3x3_sp_s2 reads a SplitMap or a SparseCanvas")
    _need_gpu(x.data, w_split, bias)
    with _Timed("conv3x3_sp_s2"):
        if w_skip is None:
            hip.check(L.coalign_conv3x3_sp_s2(_ptr(x.data), _ptr(w_split), _ptr(b), _ptr(out.data), N, Cin, cout, H, W, int(relu), flag, _stream()), "coalign_conv3x3_sp_s2")
        else:
            hip.check(L.coalign_conv3x3_sp_s2_skip(_ptr(x.data), _ptr(w_split), _ptr(b), _ptr(w_skip), _ptr(out.data), _ptr(skip), N, Cin, cout, H, W, int(relu), flag, _stream()),
                      "coalign_conv3x3_sp_s2_skip")
    return out if w_skip is None else (out, skip)


def conv3x3_sp_is_split(N: int, Cin: int, cout: int, H: int, W: int, geometry: int = 0) -> bool:
    """True when ``conv3x3_sp`` cuts this shape's tiles between workgroups (stream-K: another, still deterministic, summation order)."""
    return hip.lib().coalign_conv3x3_sp_workspace_bytes(N, Cin, cout, H, W, int(geometry)) > 0


def pack_conv3x3_wino_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] fp32 (BatchNorm folded) -> the operand image of ``coalign_conv3x3_wino`` (include/coalign_amd_lab.h, laboratory library), uint8:
    U = G g G^T in float64, split into three bf16 terms (term 0 = bf16(U), term 1 = bf16(U - term 0), term 2 = bf16(U - term 0 - term 1), the
    residuals exact in float64), stored [Cout / 64][Cin / 16][h][wave = 4 c + i][jj][term][lane][8]: the 16 bytes lane ``l`` of wavefront (i, c) loads for
    transform position (i, 2 h + jj) are U[i, 2 h + jj, 64 g + 32 c + l % 32, 16 k + 8 (l // 32) : + 8]."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or co % 64 or ci % 16:
        raise ValueError(f"conv3x3_wino needs 3x3 weights with Cout % 64 == 0 and Cin % 16 == 0, got {tuple(weight.shape)}")
    Gm = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=weight.device)
    U = torch.einsum("ia,ocab,jb->ijoc", Gm, weight.detach().double(), Gm)                 # [4 i, 4 j, Cout, Cin]
    parts, rest = [], U
    for _ in range(3):
        t = rest.float().bfloat16()
        parts.append(t)
        rest = rest - t.double()
    T = torch.stack(parts, 0)                                                              # [term, i, j, Cout, Cin] bf16
    T = T.view(3, 4, 2, 2, co // 64, 2, 32, ci // 16, 2, 8)                                # [term, i, h, jj, g, c, m, k, half, e]
    img = T.permute(4, 7, 2, 5, 1, 3, 0, 8, 6, 9).contiguous()                             # [g, k, h, c, i, jj, term, half, m, e]
    out = torch.cat([img.view(torch.uint8).reshape(-1), torch.zeros(16, dtype=torch.uint8, device=img.device)])      # + 16 zero bytes (zero padding source)
    assert out.numel() == hip.lab_lib().coalign_conv3x3_wino_weight_bytes(ci, co)
    return out


def nhwc_memory(t: torch.Tensor) -> bool:
    """A 4-d float32 tensor of logical shape [N, C, H, W] whose memory is dense [N, H, W, C]."""
    return t.dim() == 4 and t.dtype == torch.float32 and t.permute(0, 2, 3, 1).is_contiguous()


def to_nhwc(t: torch.Tensor) -> torch.Tensor:
    return t if nhwc_memory(t) else t.float().contiguous(memory_format=torch.channels_last)


@_device_op
def conv3x3_wino(x: torch.Tensor, u_split: torch.Tensor, bias: torch.Tensor, cout: int, residual: Optional[torch.Tensor] = None,
                 relu: bool = True, tile_block_w: int = 0) -> torch.Tensor:
    """y = act(conv3x3(x, w, stride 1, padding 1) + bias (+ residual)) as Winograd F(2x2, 3x3) on the split-bf16 matrix cores
    (csrc/conv3x3_wino.hip).  x / residual / y: logical [N, C, H, W] in channels-last memory (x and residual are converted if they are not)."""
    _need_gpu(x, u_split, bias, residual)
    L = hip.lab_lib()          # laboratory library only (include/coalign_amd_lab.h)
    xc = to_nhwc(x)
    N, Cin, H, W = xc.shape
    if u_split.numel() != L.coalign_conv3x3_wino_weight_bytes(Cin, cout):
        raise ValueError("transformed weight image does not match (Cin, Cout)")
    y = torch.empty((N, cout, H, W), dtype=torch.float32, device=xc.device, memory_format=torch.channels_last)
    if not nhwc_memory(y):                                 # (C == 1 or H * W == 1 cannot occur here: Cout % 64 == 0)
        y = torch.empty((N, H, W, cout), dtype=torch.float32, device=xc.device).permute(0, 3, 1, 2)
    res = None if residual is None else to_nhwc(residual)
    if res is not None and res.shape != y.shape:
        raise ValueError("residual shape mismatch")
    with _Timed("conv3x3_wino"):
        hip.check(L.coalign_conv3x3_wino(_ptr(xc), _ptr(u_split), _ptr(_f32c(bias)), _ptr(res), _ptr(y), N, Cin, cout, H, W, int(relu),
                                         int(tile_block_w), _stream()), "coalign_conv3x3_wino")
    return y


def pack_pointwise_weight(weight: torch.Tensor, transposed: bool) -> torch.Tensor:
    """ConvTranspose2d weight [Cin, Cout, k, k] -> [Cin, Cout * k * k] (a view of the same layout); Conv2d 1x1 weight
    [Cout, Cin, 1, 1] -> [Cin, Cout padded to a multiple of 32] (zero columns)."""
    w = weight.detach().float()
    if transposed:
        return w.reshape(w.shape[0], -1).contiguous()
    co, ci = w.shape[0], w.shape[1]
    out = torch.zeros((ci, (co + 31) // 32 * 32), dtype=torch.float32, device=w.device)
    out[:, :co] = w.reshape(co, ci).t()
    return out


def pack_pointwise_emu_weight(w_packed: torch.Tensor) -> torch.Tensor:
    """[Cin, M] fp32 (``pack_pointwise_weight``; Cin % 16 == 0, M % 32 == 0) -> the pre-split operand image of ``coalign_pointwise_conv_emu``
    (include/coalign_amd.h): int16 [M / 32, Cin / 16, 3 terms, 64 lanes, 8] = the bf16 bit patterns of term t of
    W[16 step + 8 (lane // 32) + j, 32 tile + lane % 32].  Terms: bf16(w), bf16(w - h), bf16(w - h - m), round-to-nearest-even (torch's
    float32 -> bfloat16 conversion, the rounding of v_cvt_pk_bf16_f32)."""
    w = w_packed.detach().float()
    Cin, M = w.shape
    if Cin % 16 or M % 32:
        raise ValueError("pointwise emu weights: Cin % 16 == 0 and M % 32 == 0")
    h = w.to(torch.bfloat16)
    r1 = w - h.float()
    m = r1.to(torch.bfloat16)
    lo = (r1 - m.float()).to(torch.bfloat16)
    terms = torch.stack([h, m, lo], 0).view(torch.int16)                       # [3, Cin, M]
    img = terms.view(3, Cin // 16, 2, 8, M // 32, 32)                           # [t, step, half, j, tile, row]
    img = img.permute(4, 1, 0, 2, 5, 3).contiguous()                           # [tile, step, t, half, row, j]
    return img.view(M // 32, Cin // 16, 3, 64, 8)


@_device_op
def pointwise_conv(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, cout: int, up: int = 1, in_stride: int = 1, relu: bool = True,
                   out: Optional[torch.Tensor] = None, c_off: int = 0, out_channels_last: bool = False) -> torch.Tensor:
    """One-launch pointwise layer (include/coalign_amd.h (10)): ``up`` > 1 = non-overlapping transposed convolution, ``in_stride`` 2 =
    1x1 stride-2 convolution.  ``out`` [N, Ctot, H', W'] + ``c_off`` select a channel slice of a larger (concatenated) tensor.
    ``w_packed``: [Cin, M] float32 (fp32 matrix cores) or the int16 image of ``pack_pointwise_emu_weight`` (split-bf16 matrix cores)."""
    _need_gpu(x, w_packed, bias)
    emu = w_packed.dtype == torch.int16
    L = hip.lib()
    nhwc = x.dtype == torch.float32 and is_channels_last(x) and x.shape[1] % 4 == 0        # read in place, no NCHW copy
    xc = x if nhwc else _f32c(x)
    N, Cin, Hin, Win = xc.shape
    Ho, Wo = (Hin + in_stride - 1) // in_stride * up, (Win + in_stride - 1) // in_stride * up
    if isinstance(out, SplitMap):                          # round 5: the layer writes its channel slice of a SplitMap (the shrink header's input)
        if not emu or out_channels_last or tuple(out.shape[2:]) != (Ho, Wo) or out.shape[0] != N or cout % 16 or c_off % 16 or c_off + cout > out.shape[1]:
            raise ValueError("SplitMap output: split-bf16 weight image, [N, Ctot, Ho, Wo] map, Cout and c_off multiples of 16")
        if w_packed.dim() != 5 or w_packed.shape[1] * 16 != Cin or not w_packed.is_contiguous() or w_packed.shape[0] * 32 != cout * up * up:
            raise ValueError("split weight image does not match (Cin, Cout * up * up)")
        with _Timed("pointwise_conv"):
            hip.check(L.coalign_pointwise_conv_emu_sp(_ptr(xc), _ptr(w_packed), _ptr(_f32c(bias)), _ptr(out.data), N, Cin, Hin, Win, in_stride, cout, up, w_packed.shape[0] * 32,
                                                      out.shape[1], c_off, int(relu), int(nhwc), _ptr(sp_range_flag(xc.device)), _stream()), "coalign_pointwise_conv_emu_sp")
        return out
    if out_channels_last:                                  # (up = 1) a fresh [N, cout, Ho, Wo] tensor in channels-last memory
        if out is not None or up != 1 or cout % 4:
            raise ValueError("channels-last output: up = 1, Cout % 4 == 0, no output slice")
        out = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=xc.device, memory_format=torch.channels_last)
    elif out is None:
        out = torch.empty((N, cout, Ho, Wo), dtype=torch.float32, device=xc.device)
    if tuple(out.shape[2:]) != (Ho, Wo) or out.shape[0] != N or not (nhwc_memory(out) if out_channels_last else out.is_contiguous()) or out.dtype != torch.float32:
        raise ValueError("output buffer shape / layout mismatch")
    nhwc_flags = int(nhwc) | (2 if out_channels_last else 0)
    with _Timed("pointwise_conv"):
        if emu:
            if w_packed.dim() != 5 or w_packed.shape[1] * 16 != Cin or not w_packed.is_contiguous():
                raise ValueError("split weight image does not match Cin")
            hip.check(L.coalign_pointwise_conv_emu(_ptr(xc), _ptr(w_packed), _ptr(_f32c(bias)), _ptr(out), N, Cin, Hin, Win, in_stride, cout, up,
                                                   w_packed.shape[0] * 32, out.shape[1], c_off, int(relu), nhwc_flags, _stream()), "coalign_pointwise_conv_emu")
        else:
            hip.check(L.coalign_pointwise_conv_ex(_ptr(xc), _ptr(w_packed), _ptr(_f32c(bias)), _ptr(out), N, Cin, Hin, Win, in_stride, cout, up,
                                                  w_packed.shape[1], out.shape[1], c_off, int(relu), nhwc_flags, _stream()), "coalign_pointwise_conv")
    return out


@_device_op
def pointwise_heads_split(layers, out: "SplitMap", relu: bool = True) -> "SplitMap":
    """The up-sampling heads of all scales in ONE launch (``coalign_pointwise_conv_emu_sp_multi``, include/coalign_amd.h (10d)): ``layers`` = [(x, w_emu, bias, cout,
    up, c_off), ...] (at most four), each writing its channel slice of the SplitMap ``out``.  Bit-identical to one ``pointwise_conv(..., out=out)`` per layer."""
    L = hip.lib()
    n = len(layers)
    N = out.shape[0]
    keep, xs, ws, bs = [], [], [], []
    ci, hi, wi, co, ups, offs, nh = [], [], [], [], [], [], []
    for (x, w_emu, bias, cout, up, c_off) in layers:
        _need_gpu(x, w_emu, bias)
        nhwc = x.dtype == torch.float32 and is_channels_last(x) and x.shape[1] % 4 == 0
        xc = x if nhwc else _f32c(x)
        b = _f32c(bias)
        if w_emu.dtype != torch.int16 or w_emu.dim() != 5 or w_emu.shape[1] * 16 != xc.shape[1] or not w_emu.is_contiguous() or w_emu.shape[0] * 32 != cout * up * up or xc.shape[0] != N:
            raise ValueError("pointwise_heads_split: split weight image of (Cin, Cout * up * up), one batch size")
        keep += [xc, b]
        xs.append(xc.data_ptr()); ws.append(w_emu.data_ptr()); bs.append(b.data_ptr())
        ci.append(xc.shape[1]); hi.append(xc.shape[2]); wi.append(xc.shape[3]); co.append(cout); ups.append(up); offs.append(c_off); nh.append(int(nhwc))
    arr_p = lambda v: (ctypes.c_void_p * n)(*v)
    arr_i = lambda v: (ctypes.c_int32 * n)(*v)
    with _Timed("pointwise_heads_split"):
        hip.check(L.coalign_pointwise_conv_emu_sp_multi(n, arr_p(xs), arr_p(ws), arr_p(bs), arr_i(ci), arr_i(hi), arr_i(wi), arr_i(co), arr_i(ups), arr_i(offs), arr_i(nh), _ptr(out.data),
                                                        N, out.shape[1], int(relu), _ptr(sp_range_flag(out.device)), _stream()), "coalign_pointwise_conv_emu_sp_multi")
    return out


HEADS_SP_MAX_ROWS = 32                             # coalign_heads_sp: the merged heads' rows fill half of one 64-row weight tile


def pack_heads_sp_weight(weight: torch.Tensor) -> torch.Tensor:
    """[M <= 32, Cin(, 1, 1)] merged head weights -> the image ``heads_sp`` reads (include/coalign_amd.h (10e)): ``pack_conv1x1_sp_weight`` of the weights padded to 64 rows."""
    w = weight.detach().float().reshape(weight.shape[0], weight.shape[1])
    if w.shape[0] > HEADS_SP_MAX_ROWS:
        raise ValueError("heads_sp serves at most 32 head channels")
    pad = torch.zeros((64, w.shape[1]), dtype=torch.float32, device=w.device)
    pad[: w.shape[0]] = w
    return pack_conv1x1_sp_weight(pad)


@_device_op
def heads_sp(x: "SplitMap", w_sp: torch.Tensor, bias: torch.Tensor, M: int) -> torch.Tensor:
    """The merged 1 x 1 heads on a SplitMap (``coalign_heads_sp``, (10e)): -> [N, M, H, W] float32, no activation."""
    if not isinstance(x, SplitMap):
        raise TypeError("heads_sp reads a SplitMap")
    _need_gpu(x.data, w_sp, bias)
    L = hip.lib()
    N, Cin, H, W = x.shape
    if w_sp.numel() != L.coalign_conv1x1_sp_weight_bytes(Cin, 64):
        raise ValueError("heads_sp: the weight image does not match Cin")
    y = torch.empty((N, M, H, W), dtype=torch.float32, device=x.device)
    with _Timed("heads_sp"):
        hip.check(L.coalign_heads_sp(_ptr(x.data), _ptr(w_sp), _ptr(_f32c(bias)), _ptr(y), N, Cin, M, H, W, _stream()), "coalign_heads_sp")
    return y


@_device_op
def boxes_overlap_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """OpenPCDet-semantics fp32 BEV overlap AREA matrix [Na, Nb] of (x, y, z, dx, dy, dz, heading) boxes."""
    _need_gpu(boxes_a, boxes_b)
    L = hip.lib()
    a, b = _f32c(boxes_a), _f32c(boxes_b)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    hip.check(L.coalign_boxes_overlap_bev(_ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out), _stream()), "coalign_boxes_overlap_bev")
    return out


@_device_op
def pcdet_nms(boxes_sorted: torch.Tensor, thresh: float, normal: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """boxes_sorted [n, 7] (descending score order) -> (keep int32 [n] positions, keep_count int32 [1]), both on the device."""
    _need_gpu(boxes_sorted)
    L = hip.lib()
    b = _f32c(boxes_sorted)
    n = b.shape[0]
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=b.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=b.device)
    ws_bytes = L.coalign_pcdet_nms_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=b.device)
    hip.check(L.coalign_pcdet_nms(_ptr(b), n, float(thresh), int(normal), _ptr(keep), _ptr(cnt), _ptr(ws), ws_bytes, _stream()), "coalign_pcdet_nms")
    return keep, cnt


# ---- DiscoNet's pixel-weight fusion (include/coalign_amd_disco.h, csrc/disco_fuse.hip) ---------------------------------------------------------------
DISCO_MAX_CHANNELS = 384


def disco_fuse_shape_ok(channels: int, n_agents: int) -> bool:
    """The shapes ``coalign_disco_fuse`` takes: C % 32 == 0, 32 <= C <= 384, 1 .. 8 agents (any H, W)."""
    return channels % 32 == 0 and 32 <= channels <= DISCO_MAX_CHANNELS and 1 <= n_agents <= 8


def _sp16_pair(w: torch.Tensor):
    """float32 -> the sp16 pair of csrc/common.h as the host makes it for weights: w~ = w rounded to 22 significant bits, h = fp16(w~) to nearest, l = (w~ - h) * 2^10."""
    ws = ((w.contiguous().view(torch.int32) + 2) & -4).view(torch.float32)
    hi = ws.half()
    return hi, ((ws - hi.float()) * 1024.0).half()


def _disco_operand_image(w: torch.Tensor) -> torch.Tensor:
    """w [R, K] (R % 32 == 0, K % 16 == 0) -> bytes of [K / 16 steps][R / 32 row tiles][64 lanes][8 h | 8 l] fp16, lane (r, half) of a (step, tile) holding
    w[32 tile + r][16 step + 8 half + j]: the A operand of v_mfma_f32_32x32x16_f16 as one contiguous 32-byte piece per lane."""
    R, K = w.shape

    def lanes(t):      # [tile, r, step, half, j] -> [step, tile, half, r, j]
        return t.reshape(R // 32, 32, K // 16, 2, 8).permute(2, 0, 3, 1, 4)
    hi, lo = _sp16_pair(w)
    return torch.stack([lanes(hi), lanes(lo)], dim=4).contiguous().view(torch.uint8).reshape(-1)


def pack_disco_weights(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, w4: torch.Tensor,
                       b4: torch.Tensor) -> Optional[torch.Tensor]:
    """The folded PixelWeightLayer (w1 [128, 2C], w2 [32, 128], w3 [8, 32], w4 [8], biases) -> the parameter image of ``coalign_disco_fuse`` (layout: the header's
    (11a)), a uint8 tensor on the weights' device; None when a weight of the two matrix layers lies outside the fp16 range (its sp16 pair would saturate)."""
    w1, w2, w3 = w1.detach().float().reshape(128, -1), w2.detach().float().reshape(32, 128), w3.detach().float().reshape(8, 32)
    C = w1.shape[1] // 2
    if not disco_fuse_shape_ok(C, 1) or not bool(torch.isfinite(w1).all() and torch.isfinite(w2).all()) or max(float(w1.abs().max()), float(w2.abs().max())) > 65504.0:
        return None
    w3p = w3.reshape(8, 4, 2, 4).permute(2, 0, 1, 3).reshape(-1)      # [half][row][q = 4 i + j] <- column 8 i + 4 half + j: the order of a lane's 16 result registers
    floats = torch.cat([t.detach().float().reshape(-1) for t in (b1, b2, w3p, b3, w4, b4)] + [w1.new_zeros(3)])
    img = torch.cat([_disco_operand_image(w1[:, :C]), _disco_operand_image(w1[:, C:]), _disco_operand_image(w2), floats.contiguous().view(torch.uint8)])
    assert img.numel() == 2 * (C // 16) * 8192 + 16384 + 436 * 4
    return img.contiguous()


@_device_op
def disco_fuse(x: torch.Tensor, theta: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """DiscoFusion of ONE frame in one launch: x [n <= 8, C, H, W] float32 in channels-last memory (agent 0 the ego), theta [n, 2, 3] (row 0 of the frame's
    normalised affine matrix), params from ``pack_disco_weights`` -> the fused map [1, C, H, W], channels-last."""
    _need_gpu(x, theta, params)
    L = hip.lib()
    n, C, H, W = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous(memory_format=torch.channels_last) or not disco_fuse_shape_ok(C, n):
        raise ValueError("disco_fuse needs a channels-last float32 map [1 .. 8 agents, C % 32 == 0 in 32 .. 384, H, W]")
    th = theta.to(device=x.device, dtype=torch.float64).contiguous()
    if th.shape[0] != n:
        raise ValueError("one theta row per agent")
    out = torch.empty((1, C, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with _Timed("disco_fuse"):
        hip.check(L.coalign_disco_fuse(_ptr(x), n, C, H, W, _ptr(th), _ptr(params), params.numel(), _ptr(out), _stream()), "coalign_disco_fuse")
    return out


# ---- V2VNet's message passing between its convolutions (include/coalign_amd_v2v.h, csrc/v2v_fuse.hip) -------------------------------------------------
V2V_AGG = {"max": 0, "avg": 1}                     # COALIGN_V2V_AGG_*
V2V_OUT_NHWC, V2V_OUT_SP = 0, 1                    # COALIGN_V2V_OUT_*


def v2v_shape_ok(channels: int, n_agents: int) -> bool:
    """The shapes the three ``coalign_v2v_*`` kernels take: C % 16 == 0, 1 .. 8 agents (any H, W)."""
    return channels > 0 and channels % 16 == 0 and 1 <= n_agents <= 8


def _nhwc_map(t: torch.Tensor, what: str) -> Tuple[int, int, int, int]:
    if t.dtype != torch.float32 or t.dim() != 4 or not nhwc_memory(t):
        raise ValueError(f"{what}: a float32 map [N, C, H, W] in channels-last memory")
    return tuple(t.shape)


def _theta_pairs(theta: torch.Tensor, n: int, device) -> torch.Tensor:
    th = theta.to(device=device, dtype=torch.float64).contiguous()
    if th.dim() != 4 or th.shape[1] != n or tuple(th.shape[2:]) != (2, 3) or not 1 <= th.shape[0] <= n:
        raise ValueError("theta: [R <= n, n, 2, 3], row (i, j) receiver i's grid in sender j")
    return th


def _nhwc_empty(N: int, C: int, H: int, W: int, device) -> torch.Tensor:
    return torch.empty((N, H, W, C), dtype=torch.float32, device=device).permute(0, 3, 1, 2)


@_device_op
def v2v_warp_split(x: torch.Tensor, theta: torch.Tensor) -> "SplitMap":
    """``SplitMap`` [R n, C, H, W] of ``warp_affine_simple(x[j], theta[i, j])`` at index i n + j in one pass (``coalign_v2v_warp_split``): x [n <= 8, C, H, W]
    float32 channels-last, theta [R <= n, n, 2, 3].  Bit for bit ``SplitMap.pack(warp_fuse_nhwc([x], theta[i], FUSE_NONE)[0])`` per receiver."""
    _need_gpu(x, theta)
    n, C, H, W = _nhwc_map(x, "v2v_warp_split")
    if not v2v_shape_ok(C, n):
        raise ValueError("v2v_warp_split: C % 16 == 0, 1 .. 8 agents")
    th = _theta_pairs(theta, n, x.device)
    R = th.shape[0]
    out = SplitMap.empty(R * n, C, H, W, x.device)
    with _Timed("v2v_warp_split"):
        hip.check(hip.lib().coalign_v2v_warp_split(_ptr(x), n, R, C, H, W, _ptr(th), _ptr(out.data), _ptr(sp_range_flag(x.device)), _stream()), "coalign_v2v_warp_split")
    return out


@_device_op
def v2v_aggregate(a: torch.Tensor, e: torch.Tensor, x: torch.Tensor, theta: torch.Tensor, agg: str = "max", gru: bool = True):
    """m_ij = (a[i n + j] + e[i]) * mask_ij, agg_i = max_j / mean_j m_ij (``coalign_v2v_aggregate``); ``gru``: the SplitMap [R, 2C, H, W] of [x_i | agg_i], else the
    float32 channels-last map x_i + agg_i.  a [R n, C, H, W], e [R, C, H, W], x [>= R, C, H, W] float32 channels-last, theta [R, n, 2, 3]."""
    _need_gpu(a, e, x, theta)
    if agg not in V2V_AGG:
        raise ValueError("agg_operator has wrong value")
    R, C, H, W = _nhwc_map(e, "v2v_aggregate e")
    Rn = _nhwc_map(a, "v2v_aggregate a")[0]
    n = Rn // max(R, 1)
    th = _theta_pairs(theta, n, e.device)
    if not v2v_shape_ok(C, n) or tuple(a.shape) != (R * n, C, H, W) or th.shape[0] != R or _nhwc_map(x, "v2v_aggregate x")[1:] != (C, H, W) or x.shape[0] < R:
        raise ValueError("v2v_aggregate: a [R n, C, H, W], e [R, C, H, W], x [>= R, C, H, W], theta [R, n, 2, 3], C % 16 == 0, n <= 8")
    out = SplitMap.empty(R, 2 * C, H, W, e.device) if gru else _nhwc_empty(R, C, H, W, e.device)
    with _Timed("v2v_aggregate"):
        hip.check(hip.lib().coalign_v2v_aggregate(_ptr(a), _ptr(e), _ptr(x), n, R, C, H, W, _ptr(th), V2V_AGG[agg], V2V_OUT_SP if gru else V2V_OUT_NHWC,
                                                  _ptr(out.data if gru else out), _ptr(sp_range_flag(e.device)) if gru else None, _stream()), "coalign_v2v_aggregate")
    return out


@_device_op
def v2v_gate(y: torch.Tensor, out_split: bool = False):
    """sigmoid(y[:, :Ch]) * tanh(y[:, Ch:]) (``coalign_v2v_gate``): y [R, 2 Ch, H, W] float32 channels-last -> float32 channels-last [R, Ch, H, W] or its SplitMap."""
    _need_gpu(y)
    R, C2, H, W = _nhwc_map(y, "v2v_gate")
    if C2 % 32:
        raise ValueError("v2v_gate: Ch % 16 == 0")
    Ch = C2 // 2
    out = SplitMap.empty(R, Ch, H, W, y.device) if out_split else _nhwc_empty(R, Ch, H, W, y.device)
    with _Timed("v2v_gate"):
        hip.check(hip.lib().coalign_v2v_gate(_ptr(y), R, Ch, H, W, V2V_OUT_SP if out_split else V2V_OUT_NHWC, _ptr(out.data if out_split else out),
                                             _ptr(sp_range_flag(y.device)) if out_split else None, _stream()), "coalign_v2v_gate")
    return out


# ---- V2X-ViT's heterogeneous agent attention (include/coalign_amd_v2x.h, csrc/v2x_attn.hip) ------------------------------------------------------------
V2X_DIM_HEAD = 32


def v2x_attn_shape_ok(channels: int, heads: int, dim_head: int, n_agents: int = 1) -> bool:
    """The shapes ``coalign_v2x_agent_attention`` takes: C = heads x 32 = 256 or 64, 1 .. 8 agents (any H, W)."""
    return channels in (64, 256) and dim_head == V2X_DIM_HEAD and heads * dim_head == channels and 1 <= n_agents <= 8


def _v2x_value_bound(w: torch.Tensor, b: torch.Tensor) -> float:
    """max_r ||w_r||_2 sqrt(C) + |b_r| in float64 over the rows of a folded value projection w [rows, C], b [rows]: with sum yhat^2 <= C (yhat = (x - mean) /
    sqrt(var + eps)) no token's |w yhat + b|_r exceeds it (Cauchy-Schwarz), and a softmax-weighted mean of such rows does not either.  NaN / inf when the
    operands are not finite (a comparison ``< 65504`` is then false)."""
    w, b = w.detach().double(), b.detach().double().reshape(-1)
    return float((w.norm(dim=1) * float(w.shape[1]) ** 0.5 + b.abs()).max())


def pack_v2x_weights(wqkv: torch.Tensor, bqkv: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor) -> Optional[torch.Tensor]:
    """The folded agent-attention layer (wqkv [3C, C] = [q | k' | v'] rows, bqkv [3C], wa [C, C], ba [C]) -> the parameter image of ``coalign_v2x_agent_attention``
    (layout: the header's (13a)), a uint8 tensor on the weights' device.  None when a weight lies outside the fp16 range (its sp16 pair would saturate), or when
    an attention output could reach its end: o is a convex combination of the senders' v' rows and enters the output projection as fp16 pairs, and
    |v'|_r <= ``_v2x_value_bound`` for every token -- a static guarantee in place of a device flag, as ``pack_v2x_ffn_weights`` gives."""
    wqkv, wa = wqkv.detach().float(), wa.detach().float()
    C = wa.shape[0]
    if tuple(wqkv.shape) != (3 * C, C) or tuple(wa.shape) != (C, C) or C not in (64, 256) or bqkv.numel() != 3 * C:
        raise ValueError("pack_v2x_weights: wqkv [3C, C], bqkv [3C], wa [C, C], C = 64 or 256")
    if not bool(torch.isfinite(wqkv).all() and torch.isfinite(wa).all()) or max(float(wqkv.abs().max()), float(wa.abs().max())) > 65504.0:
        return None
    if not _v2x_value_bound(wqkv[2 * C:], bqkv.detach().reshape(-1)[2 * C:]) < 65504.0:
        return None
    floats = torch.cat([bqkv.detach().float().reshape(-1), ba.detach().float().reshape(-1)])
    img = torch.cat([_disco_operand_image(wqkv), _disco_operand_image(wa), floats.contiguous().view(torch.uint8)])
    assert img.numel() == (C // 16) * (4 * C // 32) * 2048 + 16 * C
    return img.contiguous()


@_device_op
def v2x_agent_attention(x: torch.Tensor, theta: Optional[torch.Tensor], params: torch.Tensor, receivers: Optional[int] = None) -> torch.Tensor:
    """x + HGTCavAttention(LayerNorm(x)) over the agents of ONE frame (``coalign_v2x_agent_attention``): x [n <= 8, H, W, C] float32 contiguous (agent 0 the ego),
    theta [n, 2, 3] (row 0 of the frame's normalised affine matrix: x is warped first) or None (x is read in place), params from ``pack_v2x_weights``,
    ``receivers`` R = n (default) or 1 -> [R, H, W, C] float32."""
    _need_gpu(x, params) if theta is None else _need_gpu(x, theta, params)
    L = hip.lib()
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("v2x_agent_attention needs a contiguous float32 map [n, H, W, C]")
    n, H, W, C = x.shape
    R = n if receivers is None else int(receivers)
    if C not in (64, 256) or not 1 <= n <= 8 or R not in (1, n):
        raise ValueError("v2x_agent_attention: C = 64 or 256, 1 .. 8 agents, receivers = n or 1")
    th = None
    if theta is not None:
        th = theta.to(device=x.device, dtype=torch.float64).contiguous()
        if tuple(th.shape) != (n, 2, 3):
            raise ValueError("one theta row per agent")
    ws_bytes = int(L.coalign_v2x_workspace_bytes(n, C, H, W))
    ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((R, H, W, C), dtype=torch.float32, device=x.device)
    with _Timed("v2x_agent_attention"):
        hip.check(L.coalign_v2x_agent_attention(_ptr(x), n, R, C, H, W, _ptr(th), _ptr(params), params.numel(), _ptr(out), _ptr(ws), ws_bytes, _stream()),
                  "coalign_v2x_agent_attention")
    return out


# ---- V2X-ViT's pyramid window attention with split attention (include/coalign_amd_v2x_window.h, csrc/v2x_window.hip) -----------------------------------
V2X_WINDOWS, V2X_WINDOW_DIM_HEADS = (4, 8, 16), (16, 32, 64)
V2X_WINDOW_FUSE = {"naive": 0, "split_attn": 1}      # COALIGN_V2X_WINDOW_FUSE_*
V2X_WINDOW_POS_FLOATS = 1236


def v2x_window_shape_ok(channels: int, heads, dim_heads, windows, fuse: str, relative: bool, n_agents: int = 1, hw=None) -> bool:
    """The shapes ``coalign_v2x_window_attention`` takes: windows (4, 8, 16) with dim_head (16, 32, 64) and heads C / dim_head, a relative position table, C = 256,
    or C = 64 with ``naive``, 1 .. 8 maps, H and W (when given) multiples of 16."""
    if tuple(windows) != V2X_WINDOWS or tuple(dim_heads) != V2X_WINDOW_DIM_HEADS or tuple(heads) != tuple(channels // d for d in V2X_WINDOW_DIM_HEADS):
        return False
    if not relative or fuse not in V2X_WINDOW_FUSE or not (channels == 256 or (channels == 64 and fuse == "naive")) or not 1 <= n_agents <= 8:
        return False
    return hw is None or (int(hw[0]) > 0 and int(hw[1]) > 0 and int(hw[0]) % 16 == 0 and int(hw[1]) % 16 == 0)


def pack_v2x_window_weights(wqkv: torch.Tensor, bqkv: torch.Tensor, wout: torch.Tensor, bout: torch.Tensor, pos: Sequence[torch.Tensor], split=None) -> Optional[torch.Tensor]:
    """The folded window-attention layer (``v2xvit.folded_window_attention``: wqkv [9C, C], bqkv [9C], wout [3, C, C], bout [3, C], pos = the three position tables;
    ``split`` = (fc1.weight, bn1.weight, bn1.bias, fc2.weight) of the split attention or None for ``naive``) -> the parameter image of
    ``coalign_v2x_window_attention`` (layout: the header's (14a)), a uint8 tensor on the weights' device.  None when a weight of the matrix layers lies outside the
    fp16 range (its sp16 pair would saturate), or when an attention output could reach its end: o_b is a convex combination of branch b's v rows and enters the
    output projection as fp16 pairs, and |v_b|_r <= ``_v2x_value_bound`` for every token -- a static guarantee in place of a device flag."""
    wqkv, wout = wqkv.detach().float(), wout.detach().float()
    C = wout.shape[-1]
    if (tuple(wqkv.shape) != (9 * C, C) or tuple(wout.shape) != (3, C, C) or not (C == 256 or (C == 64 and split is None)) or bqkv.numel() != 9 * C
            or [tuple(p.shape) for p in pos] != [(7, 7), (15, 15), (31, 31)]):
        raise ValueError("pack_v2x_window_weights: wqkv [9C, C], bqkv [9C], wout [3, C, C], tables 7 x 7, 15 x 15, 31 x 31, C = 256 or (naive) 64")
    if not bool(torch.isfinite(wqkv).all() and torch.isfinite(wout).all()) or max(float(wqkv.abs().max()), float(wout.abs().max())) > 65504.0:
        return None
    bflat = bqkv.detach().reshape(-1)
    if not all(_v2x_value_bound(wqkv[3 * C * b + 2 * C:3 * C * (b + 1)], bflat[3 * C * b + 2 * C:3 * C * (b + 1)]) < 65504.0 for b in range(3)):
        return None
    floats = [bqkv.detach().float().reshape(-1), bout.detach().float().reshape(-1)] + [p.detach().float().reshape(-1) for p in pos] + [wqkv.new_zeros(1)]
    if split is not None:
        fc1, g, b, fc2 = (t.detach().float() for t in split)
        floats += [wout.transpose(1, 2).reshape(-1), fc1.t().reshape(-1), g.reshape(-1), b.reshape(-1), fc2.t().reshape(-1)]
    img = torch.cat([_disco_operand_image(wqkv)] + [_disco_operand_image(w) for w in wout] + [torch.cat(floats).contiguous().view(torch.uint8)])
    assert img.numel() == (C // 16) * (12 * C // 32) * 2048 + (12 * C + V2X_WINDOW_POS_FLOATS) * 4 + (0 if split is None else (7 * C * C + 2 * C) * 4)
    return img.contiguous()


@_device_op
def v2x_window_attention(x: torch.Tensor, params: torch.Tensor, fuse: str) -> torch.Tensor:
    """x + PyramidWindowAttention(LayerNorm(x)) for the maps of ONE frame, every map on its own (``coalign_v2x_window_attention``): x [n <= 8, H, W, C] float32
    contiguous, params from ``pack_v2x_window_weights``, ``fuse`` "naive" or "split_attn" -> [n, H, W, C] float32."""
    _need_gpu(x, params)
    L = hip.lib()
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("v2x_window_attention needs a contiguous float32 map [n, H, W, C]")
    n, H, W, C = x.shape
    if fuse not in V2X_WINDOW_FUSE or not v2x_window_shape_ok(C, [C // d for d in V2X_WINDOW_DIM_HEADS], V2X_WINDOW_DIM_HEADS, V2X_WINDOWS, fuse, True, n, (H, W)):
        raise ValueError("v2x_window_attention: C = 256 or (naive) 64, 1 .. 8 maps, H and W multiples of 16")
    ws_bytes = int(L.coalign_v2x_window_workspace_bytes(n, C, H, W))
    ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((n, H, W, C), dtype=torch.float32, device=x.device)
    with _Timed("v2x_window_attention"):
        hip.check(L.coalign_v2x_window_attention(_ptr(x), n, C, H, W, V2X_WINDOW_FUSE[fuse], _ptr(params), params.numel(), _ptr(out), _ptr(ws), ws_bytes, _stream()),
                  "coalign_v2x_window_attention")
    return out


# ---- V2X-ViT's feed-forward block in one launch (include/coalign_amd_v2x_ffn.h, csrc/v2x_ffn.hip) --------------------------------------------------------------
V2X_FFN_MAX_HIDDEN = 512      # COALIGN_V2X_FFN_MAX_HIDDEN


def v2x_ffn_shape_ok(C: int, M: int) -> bool:
    """The shapes ``coalign_v2x_feed_forward`` takes: C = 64 or 256 channels, a hidden width M % 32 == 0 with 32 <= M <= 512 (any number of tokens)."""
    return C in (64, 256) and 32 <= M <= V2X_FFN_MAX_HIDDEN and M % 32 == 0


def pack_v2x_ffn_weights(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> Optional[torch.Tensor]:
    """The folded feed-forward layer (``v2xvit.folded_feed_forward``: w1 [M, C] = W1 diag(gamma), b1 [M] = W1 beta + b1, w2 [C, M], b2 [C]) -> the parameter image of
    ``coalign_v2x_feed_forward`` (layout: the header's (16a)), a uint8 tensor on the weights' device.  None when a folded weight reaches the end of the fp16 range
    (65504), or when a hidden pre-activation could: the hidden vector enters the second product as fp16 pairs, |GELU(z)| <= |z|, and with sum yhat^2 <= C
    |w1 yhat + b1|_r <= ||w1_r||_2 sqrt(C) + |b1_r| for every token -- a static guarantee in place of a device flag."""
    w1d, b1d, w2d = w1.detach().double(), b1.detach().double().reshape(-1), w2.detach().double()
    M, C = w1d.shape
    if tuple(w2d.shape) != (C, M) or b1d.numel() != M or b2.numel() != C or not v2x_ffn_shape_ok(C, M):
        raise ValueError("pack_v2x_ffn_weights: w1 [M, C], b1 [M], w2 [C, M], b2 [C], C = 64 or 256, M % 32 == 0 in 32 .. 512")
    if not bool(torch.isfinite(w1d).all() and torch.isfinite(w2d).all() and torch.isfinite(b1d).all()):
        return None
    bound = w1d.norm(dim=1) * float(C) ** 0.5 + b1d.abs()
    if max(float(w1d.abs().max()), float(w2d.abs().max()), float(bound.max())) >= 65504.0:
        return None
    floats = torch.cat([b1.detach().float().reshape(-1), b2.detach().float().reshape(-1)])
    img = torch.cat([_disco_operand_image(w1.detach().float()), _disco_operand_image(w2.detach().float()), floats.contiguous().view(torch.uint8)])
    assert img.numel() == 2 * (C // 16) * (M // 32) * 2048 + 4 * (M + C)
    return img.contiguous()


@_device_op
def v2x_feed_forward(x: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """x + FeedForward(LayerNorm(x)) per token in one launch (``coalign_v2x_feed_forward``): x [..., C] float32 contiguous (any channels-last map), params from
    ``pack_v2x_ffn_weights`` (its size names the hidden width) -> a new tensor of x's shape."""
    _need_gpu(x, params)
    L = hip.lib()
    if x.dim() < 1 or x.dtype != torch.float32 or not x.is_contiguous() or params.dtype != torch.uint8 or not params.is_contiguous():
        raise ValueError("v2x_feed_forward needs contiguous float32 token rows [..., C] and the uint8 image of pack_v2x_ffn_weights")
    C = x.shape[-1]
    M = (params.numel() - 4 * C) // (8 * C + 4) if C in (64, 256) else 0      # bytes = 2 (C / 16) (M / 32) 2048 + 4 (M + C) = M (8 C + 4) + 4 C
    if not v2x_ffn_shape_ok(C, M) or int(L.coalign_v2x_ffn_param_bytes(C, M)) != params.numel():
        raise ValueError("v2x_feed_forward: C = 64 or 256 and an image of pack_v2x_ffn_weights for that C")
    tokens = x.numel() // C
    out = torch.empty_like(x)
    with _Timed("v2x_feed_forward"):
        hip.check(L.coalign_v2x_feed_forward(_ptr(x), tokens, C, M, _ptr(params), params.numel(), _ptr(out), _stream()), "coalign_v2x_feed_forward")
    return out


# ---- When2com's handshake fusion after its convolutions (include/coalign_amd_w2c.h, csrc/w2c_fuse.hip) ---------------------------------------------------
W2C_CHANNELS, W2C_FEAT, W2C_HIDDEN1, W2C_HIDDEN2, W2C_ATT = 128, 4480, 256, 128, 128      # COALIGN_W2C_*
W2C_PARAM_FLOATS = 2 * W2C_HIDDEN1 * W2C_FEAT + 2 * W2C_HIDDEN1 + 2 * (W2C_HIDDEN1 * W2C_HIDDEN2 + W2C_HIDDEN2) + 2 * (W2C_HIDDEN2 * W2C_ATT + W2C_ATT)


def w2c_shape_ok(channels: int, n_agents: int) -> bool:
    """The shapes ``coalign_w2c_fuse`` (and ``v2v_warp_split`` ahead of it) takes: C % 16 == 0, 1 .. 8 agents (any H, W)."""
    return channels > 0 and channels % 16 == 0 and 1 <= n_agents <= 8


def pack_w2c_weights(key_net, query_net) -> torch.Tensor:
    """The parameter image of ``coalign_w2c_score`` (layout: the header's COALIGN_W2C_PARAM_FLOATS) from two tuples ``(W1 [256, 4480], b1, W2 [128, 256], b2,
    T [128, 128], tb)`` -- fc.0, fc.2 and the folded tail of the key and the query net -- as one float32 tensor on the weights' device."""
    shapes = ((W2C_HIDDEN1, W2C_FEAT), (W2C_HIDDEN1,), (W2C_HIDDEN2, W2C_HIDDEN1), (W2C_HIDDEN2,), (W2C_ATT, W2C_HIDDEN2), (W2C_ATT,))
    nets = []
    for net in (key_net, query_net):
        if len(net) != 6 or any(tuple(t.shape) != s for t, s in zip(net, shapes)):
            raise ValueError("pack_w2c_weights: (W1 [256, 4480], b1 [256], W2 [128, 256], b2 [128], T [128, 128], tb [128]) per net")
        nets.append([t.detach().float() for t in net])
    k, q = nets
    parts = [k[0], q[0], k[1], q[1], k[2].t(), k[3], q[2].t(), q[3], k[4].t(), k[5], q[4].t(), q[5]]
    img = torch.cat([p.contiguous().reshape(-1) for p in parts]).contiguous()
    assert img.numel() == W2C_PARAM_FLOATS
    return img


_W2C_WS = {}


def _w2c_workspace(device) -> torch.Tensor:
    """The partial-sum workspace of ``coalign_w2c_score`` for the current stream of ``device`` (launches on a stream are ordered; nothing to initialise)."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _W2C_WS.get(key)
    if ws is None:
        ws = _W2C_WS[key] = torch.empty(hip.lib().coalign_w2c_workspace_bytes(), dtype=torch.uint8, device=device)
    return ws


@_device_op
def w2c_score(key: "SplitMap", query: "SplitMap", params: torch.Tensor, return_logits: bool = False):
    """The attention weights of ONE frame (``coalign_w2c_score``): key [n <= 8, 128 or more, h, w] (the key net's conv1 output in its first 128 channels) and query
    [1, 128, h, w] SplitMaps, read in place -- of a stacked key | query convolution: the 256-channel map itself and ``SplitMap(map.data[:1, 8:])``; params from
    ``pack_w2c_weights`` -> w [n] float32 on the device; ``return_logits`` (tests): (w, logits [n])."""
    if not isinstance(key, SplitMap) or not isinstance(query, SplitMap):
        raise TypeError("w2c_score reads SplitMaps")
    _need_gpu(key.data, query.data, params)
    n, C, h, w = key.shape
    if C < W2C_CHANNELS or tuple(query.shape) != (1, W2C_CHANNELS, h, w) or not 1 <= n <= 8 or query.device != key.device:
        raise ValueError("w2c_score: key [1 .. 8, >= 128, h, w], query [1, 128, h, w] on one device")
    if params.dtype != torch.float32 or params.numel() != W2C_PARAM_FLOATS or not params.is_contiguous() or params.device != key.device:
        raise ValueError("w2c_score: params is the float32 image of pack_w2c_weights on the maps' device")
    out = torch.empty(n, dtype=torch.float32, device=key.device)
    logits = torch.empty(n, dtype=torch.float32, device=key.device) if return_logits else None
    ws = _w2c_workspace(key.device)
    with _Timed("w2c_score"):
        hip.check(hip.lib().coalign_w2c_score(_ptr(key.data), C, _ptr(query.data), n, h, w, _ptr(params), params.numel() * 4, _ptr(out), _ptr(logits), _ptr(ws), ws.numel(),
                                              _stream()), "coalign_w2c_score")
    return (out, logits) if return_logits else out


@_device_op
def w2c_fuse(x: torch.Tensor, theta: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """sum_j weights[j] * warp_affine_simple(x[j], theta[j]) of ONE frame in one launch (``coalign_w2c_fuse``): x [n <= 8, C, H, W] float32 channels-last, theta
    [n, 2, 3], weights [n] float32 on the device -> [1, C, H, W] float32 channels-last."""
    _need_gpu(x, theta, weights)
    n, C, H, W = _nhwc_map(x, "w2c_fuse")
    if not w2c_shape_ok(C, n):
        raise ValueError("w2c_fuse: C % 16 == 0, 1 .. 8 agents")
    th = theta.to(device=x.device, dtype=torch.float64).contiguous()
    if tuple(th.shape) != (n, 2, 3):
        raise ValueError("w2c_fuse: theta [n, 2, 3], one row per agent")
    if weights.dtype != torch.float32 or tuple(weights.shape) != (n,) or not weights.is_contiguous() or weights.device != x.device:
        raise ValueError("w2c_fuse: weights [n] float32 on the map's device")
    out = _nhwc_empty(1, C, H, W, x.device)
    with _Timed("w2c_fuse"):
        hip.check(hip.lib().coalign_w2c_fuse(_ptr(x), n, C, H, W, _ptr(th), _ptr(weights), _ptr(out), _stream()), "coalign_w2c_fuse")
    return out


# ---- The pose-robust V2VNet between its convolutions (include/coalign_amd_v2v_robust.h, csrc/v2v_robust.hip) -------------------------------------------------
V2VR_MAX_CAV = 16


def v2vr_shape_ok(channels: int, hidden: int, n_agents: int, max_cav: int = 5) -> bool:
    """The shapes the ``coalign_v2vr_*`` kernels take: C % 16 == 0 (the maps), hidden % 64 == 0 and <= 1024 (the two heads), 1 .. 8 agents in at most 16 slots."""
    return channels > 0 and channels % 16 == 0 and hidden > 0 and hidden % 64 == 0 and hidden <= 1024 and 1 <= n_agents <= 8 and n_agents <= max_cav <= V2VR_MAX_CAV


def _f64_dev(t: torch.Tensor, shape, what: str) -> torch.Tensor:
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous float64 tensor {list(shape)}")
    return t


@_device_op
def v2vr_pool_act(a: torch.Tensor, e: Optional[torch.Tensor] = None, n: int = 1, out_split: bool = True):
    """lrelu(max_pool2d(a + e[p // n], 2)) in one pass (``coalign_v2vr_pool_act``): a [P, C, H, W], e [P / n, C, H, W] or None, float32 channels-last -> the
    SplitMap [P, C, H // 2, W // 2] or the float32 channels-last map."""
    _need_gpu(a, e)
    P, C, H, W = _nhwc_map(a, "v2vr_pool_act a")
    if C % 16 or H < 2 or W < 2 or (e is not None and (n < 1 or P % n or _nhwc_map(e, "v2vr_pool_act e") != (P // n, C, H, W))):
        raise ValueError("v2vr_pool_act: a [P, C, H, W], e [P / n, C, H, W] or None, C % 16 == 0, H and W at least 2")
    out = SplitMap.empty(P, C, H // 2, W // 2, a.device) if out_split else _nhwc_empty(P, C, H // 2, W // 2, a.device)
    with _Timed("v2vr_pool_act"):
        hip.check(hip.lib().coalign_v2vr_pool_act(_ptr(a), _ptr(e), P, int(n), C, H, W, V2V_OUT_SP if out_split else V2V_OUT_NHWC, _ptr(out.data if out_split else out),
                                                  _ptr(sp_range_flag(a.device)) if out_split else None, _stream()), "coalign_v2vr_pool_act")
    return out


@_device_op
def v2vr_score_head(y: torch.Tensor, n: int, max_cav: int, w: torch.Tensor, b: torch.Tensor, alpha: torch.Tensor):
    """The attention's tail and the aggregation weights of one frame (``coalign_v2vr_score_head``): y [n n, h, H, W] float32 channels-last (the second convolution's
    output), w [h], b [1], alpha [1] float32 on the device -> (scores [L, L], weight [L, L])."""
    _need_gpu(y, w, b, alpha)
    P, h, H, W = _nhwc_map(y, "v2vr_score_head")
    if P != n * n or not v2vr_shape_ok(16, h, n, max_cav) or H < 2 or W < 2 or any(t.dtype != torch.float32 or not t.is_contiguous() for t in (w, b, alpha)) or w.numel() != h or b.numel() != 1 or alpha.numel() != 1:
        raise ValueError("v2vr_score_head: y [n n, h, H, W], h % 64 == 0, w [h], b [1], alpha [1] float32, n <= 8, n <= max_cav <= 16")
    scores = torch.empty((max_cav, max_cav), dtype=torch.float32, device=y.device)
    weight = torch.empty_like(scores)
    with _Timed("v2vr_score_head"):
        hip.check(hip.lib().coalign_v2vr_score_head(_ptr(y), n, max_cav, h, H, W, _ptr(w), _ptr(b), _ptr(alpha), _ptr(scores), _ptr(weight), _stream()), "coalign_v2vr_score_head")
    return scores, weight


@_device_op
def v2vr_pose_head(y4: "SplitMap", n: int, max_cav: int, fc, T: torch.Tensor):
    """The pose regression's tail for all pairs of one frame (``coalign_v2vr_pose_head``): y4 the SplitMap [n n, h, H4, W4] of the strided fourth convolution,
    fc = (W1 [h, h], b1, W2 [h, h], b2, W3 [3, h], b3) float32, T [L, L, 4, 4] float64 -> (pose_corr [L, L, 3] float32, T_new [L, L, 4, 4] float64)."""
    if not isinstance(y4, SplitMap):
        raise TypeError("v2vr_pose_head reads a SplitMap")
    _need_gpu(y4.data, T, *fc)
    P, h, H4, W4 = y4.shape
    shapes = ((h, h), (h,), (h, h), (h,), (3, h), (3,))
    if P != n * n or not v2vr_shape_ok(16, h, n, max_cav) or H4 < 2 or W4 < 2 or len(fc) != 6 or any(t.dtype != torch.float32 or tuple(t.shape) != s or not t.is_contiguous() for t, s in zip(fc, shapes)):
        raise ValueError("v2vr_pose_head: y4 [n n, h, H4 >= 2, W4 >= 2], h % 64 == 0, fc = (W1 [h, h], b1, W2 [h, h], b2, W3 [3, h], b3) float32 contiguous")
    _f64_dev(T, (max_cav, max_cav, 4, 4), "v2vr_pose_head T")
    corr = torch.empty((max_cav, max_cav, 3), dtype=torch.float32, device=T.device)
    T_new = torch.empty_like(T)
    ws = torch.empty(hip.lib().coalign_v2vr_pose_head_workspace_bytes(n, h), dtype=torch.uint8, device=T.device)
    with _Timed("v2vr_pose_head"):
        hip.check(hip.lib().coalign_v2vr_pose_head(_ptr(y4.data), n, max_cav, h, H4, W4, *[_ptr(t) for t in fc], _ptr(T), _ptr(corr), _ptr(T_new), _ptr(ws), ws.numel(), _stream()),
                  "coalign_v2vr_pose_head")
    return corr, T_new


@_device_op
def v2vr_pairwise(poses: torch.Tensor, max_cav: int, H: int, W: int, den_x: float, den_y: float):
    """3-dof poses [n, 3] float64 (x, y, yaw in degrees) -> (pairwise [L, L, 4, 4], normalised affine [L, L, 2, 3]) float64 (``coalign_v2vr_pairwise``)."""
    _need_gpu(poses)
    n = poses.shape[0]
    _f64_dev(poses, (n, 3), "v2vr_pairwise poses")
    pairwise = torch.empty((max_cav, max_cav, 4, 4), dtype=torch.float64, device=poses.device)
    affine = torch.empty((max_cav, max_cav, 2, 3), dtype=torch.float64, device=poses.device)
    with _Timed("v2vr_pairwise"):
        hip.check(hip.lib().coalign_v2vr_pairwise(_ptr(poses), n, max_cav, H, W, float(den_x), float(den_y), _ptr(pairwise), _ptr(affine), _stream()), "coalign_v2vr_pairwise")
    return pairwise, affine


@_device_op
def v2vr_consistency(poses: torch.Tensor, T_new: torch.Tensor, H: int, W: int, den_x: float, den_y: float):
    """The whole ``WeightedEM`` of one frame in one launch (``coalign_v2vr_consistency``): poses [n, 3], T_new [L, L, 4, 4] float64 -> (corrected poses [n, 3],
    pairwise [L, L, 4, 4], normalised affine [L, L, 2, 3]) float64."""
    _need_gpu(poses, T_new)
    n, L = poses.shape[0], T_new.shape[0]
    _f64_dev(poses, (n, 3), "v2vr_consistency poses")
    _f64_dev(T_new, (L, L, 4, 4), "v2vr_consistency T_new")
    out = torch.empty_like(poses)
    pairwise = torch.empty_like(T_new)
    affine = torch.empty((L, L, 2, 3), dtype=torch.float64, device=poses.device)
    with _Timed("v2vr_consistency"):
        hip.check(hip.lib().coalign_v2vr_consistency(_ptr(poses), _ptr(T_new), n, L, H, W, float(den_x), float(den_y), _ptr(out), _ptr(pairwise), _ptr(affine), _stream()),
                  "coalign_v2vr_consistency")
    return out, pairwise, affine


@_device_op
def v2vr_aggregate(a: torch.Tensor, e: torch.Tensor, x: torch.Tensor, theta: torch.Tensor, weight: torch.Tensor, gru: bool = True):
    """``v2v_aggregate`` with agg_i = sum_j m_ij * weight[i, j] in order of j (``coalign_v2vr_aggregate``): weight [>= R, L] float32 on the device, rows contiguous."""
    _need_gpu(a, e, x, theta, weight)
    R, C, H, W = _nhwc_map(e, "v2vr_aggregate e")
    Rn = _nhwc_map(a, "v2vr_aggregate a")[0]
    n = Rn // max(R, 1)
    th = _theta_pairs(theta, n, e.device)
    if not v2v_shape_ok(C, n) or tuple(a.shape) != (R * n, C, H, W) or th.shape[0] != R or _nhwc_map(x, "v2vr_aggregate x")[1:] != (C, H, W) or x.shape[0] < R:
        raise ValueError("v2vr_aggregate: a [R n, C, H, W], e [R, C, H, W], x [>= R, C, H, W], theta [R, n, 2, 3], C % 16 == 0, n <= 8")
    if weight.dtype != torch.float32 or weight.dim() != 2 or weight.shape[0] < R or not n <= weight.shape[1] <= V2VR_MAX_CAV or not weight.is_contiguous() or weight.device != e.device:
        raise ValueError("v2vr_aggregate: weight [>= R, n <= L <= 16] float32 contiguous on the maps' device")
    out = SplitMap.empty(R, 2 * C, H, W, e.device) if gru else _nhwc_empty(R, C, H, W, e.device)
    with _Timed("v2vr_aggregate"):
        hip.check(hip.lib().coalign_v2vr_aggregate(_ptr(a), _ptr(e), _ptr(x), n, R, C, H, W, _ptr(th), _ptr(weight), int(weight.shape[1]), V2V_OUT_SP if gru else V2V_OUT_NHWC,
                                                   _ptr(out.data if gru else out), _ptr(sp_range_flag(e.device)) if gru else None, _stream()), "coalign_v2vr_aggregate")
    return out


# ---- Where2comm's confidence-masked fusion (include/coalign_amd_where2comm.h, csrc/w2comm.hip) ------------------------------------------------------------------
W2COMM_MAX_GROUPS, W2COMM_MAX_K, W2COMM_MAX_LEVELS, W2COMM_MAX_ANCHORS = 64, 9, 3, 8


def w2comm_masks_shape_ok(anchors: int, group_len: Sequence[int], k: int, levels: int, hw=None) -> bool:
    """What ``coalign_w2comm_masks`` takes: 1 .. 8 anchors, 1 .. 64 frames of 1 .. 8 agents, k = 0 or odd and <= 9, 1 .. 3 levels that every halving leaves a pixel."""
    ok = 1 <= anchors <= W2COMM_MAX_ANCHORS and 1 <= len(group_len) <= W2COMM_MAX_GROUPS and all(1 <= int(g) <= 8 for g in group_len)
    ok = ok and (k == 0 or (k % 2 == 1 and 0 < k <= W2COMM_MAX_K)) and 1 <= levels <= W2COMM_MAX_LEVELS
    return bool(ok and (hw is None or (hw[0] >> (levels - 1) >= 1 and hw[1] >> (levels - 1) >= 1)))


@_device_op
def w2comm_masks(psm: torch.Tensor, group_len: Sequence[int], weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], thre: float, levels: int = 1):
    """The communication masks and rates of a batch in one launch (``coalign_w2comm_masks``): psm [n_total, A, H, W] float32, the single-agent classification logits;
    ``weight`` [k, k] (any leading ones: ``gaussian_filter.weight`` as stored) and ``bias`` [1] float32 on the device, or both None for no smoothing ->
    (masks: per level l a uint8 tensor [n_total, H >> l, W >> l] of 0 / 1, rates [len(group_len)] float32)."""
    _need_gpu(psm, weight, bias)
    if psm.dim() != 4 or psm.dtype != torch.float32:
        raise ValueError("w2comm_masks: psm [n_total, A, H, W] float32")
    p = psm.contiguous()
    n_total, A, H, W = p.shape
    groups = [int(g) for g in group_len]
    k = 0
    if weight is not None:
        k = int(weight.shape[-1])
        if bias is None or weight.numel() != k * k or bias.numel() != 1 or weight.dtype != torch.float32 or bias.dtype != torch.float32 or weight.device != p.device or bias.device != p.device:
            raise ValueError("w2comm_masks: weight [k, k] and bias [1] float32 on the map's device")
        weight, bias = weight.contiguous(), bias.contiguous()
    if sum(groups) != n_total:
        raise ValueError("w2comm_masks: group_len must sum to psm's agents")
    levels = int(levels)
    masks = [torch.empty((n_total, H >> l, W >> l), dtype=torch.uint8, device=p.device) for l in range(max(0, min(levels, W2COMM_MAX_LEVELS)))]
    rates = torch.empty(len(groups), dtype=torch.float32, device=p.device)
    gl = (ctypes.c_int32 * max(1, len(groups)))(*groups)
    mp = (ctypes.c_void_p * max(1, len(masks)))(*[m.data_ptr() for m in masks])
    with _Timed("w2comm_masks"):
        hip.check(hip.lib().coalign_w2comm_masks(_ptr(p), n_total, A, H, W, gl, len(groups), _ptr(weight), _ptr(bias), k, float(thre), levels, mp, _ptr(rates),
                                                 _stream()), "coalign_w2comm_masks")
    return masks, rates


@_device_op
def w2comm_fuse_nhwc(xs: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], theta: torch.Tensor, mode: int, rows: Optional[Sequence[int]] = None) -> list:
    """``warp_fuse_nhwc`` of ONE frame on maps multiplied by their masks, without the product (``coalign_w2comm_fuse_nhwc``): ``xs[i]`` [n, C_i, H_i, W_i] channels-last
    float32, ``masks[i]`` [n, H_i, W_i] uint8 (row r belongs to row r of ``xs[i]``), theta [n, 2, 3] f64, mode FUSE_ATT / FUSE_MAX -> per scale [1, C_i, H_i, W_i]
    channels-last."""
    _need_gpu(*xs, *masks, theta)
    k = len(xs)
    n = xs[0].shape[0]
    if not 1 <= k <= 3 or any(not warp_fuse_nhwc_ok(x) or x.shape[0] != n for x in xs):
        raise ValueError("w2comm_fuse_nhwc needs 1-3 channels-last float32 maps [n <= 8, C in {64, 128, 256}, H, W] of one frame")
    if len(masks) != k or any(m.dtype != torch.uint8 or tuple(m.shape) != (n, x.shape[2], x.shape[3]) or not m.is_contiguous() or m.device != x.device for m, x in zip(masks, xs)):
        raise ValueError("w2comm_fuse_nhwc: one contiguous uint8 mask [n, H, W] per map, on the map's device")
    if mode not in (FUSE_ATT, FUSE_MAX):
        raise ValueError("w2comm_fuse_nhwc fuses (FUSE_ATT | FUSE_MAX)")
    th = theta.to(device=xs[0].device, dtype=torch.float64).contiguous()
    if th.shape[0] != n:
        raise ValueError("one theta row per agent")
    outs = [torch.empty((1, x.shape[1], x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device, memory_format=torch.channels_last) for x in xs]
    vp = ctypes.c_void_p * k
    i32 = ctypes.c_int32 * k
    rw = None
    if rows is not None:
        if len(rows) != n:
            raise ValueError("rows must have one entry per agent")
        rw = (ctypes.c_int32 * n)(*[int(r) for r in rows])
    with _Timed("w2comm_fuse_nhwc"):
        hip.check(hip.lib().coalign_w2comm_fuse_nhwc(k, vp(*[x.data_ptr() for x in xs]), i32(*[x.shape[1] for x in xs]), i32(*[x.shape[2] for x in xs]),
                                                     i32(*[x.shape[3] for x in xs]), vp(*[m.data_ptr() for m in masks]), vp(*[o.data_ptr() for o in outs]),
                                                     i32(*[x.shape[2] for x in xs]), i32(*[x.shape[3] for x in xs]), n, _ptr(th), rw, mode, _stream()),
                  "coalign_w2comm_fuse_nhwc")
    return outs


# ---- Where2comm's messages (include/coalign_amd_where2comm_msg.h, csrc/w2comm_msg.hip) -------------------------------------------------------------------------------
W2COMM_SRC_DENSE, W2COMM_SRC_PACKED = 0, 1


def w2comm_msg_shape_ok(channels: Sequence[int], n_agents: int = 1, hw: Optional[Sequence[Tuple[int, int]]] = None) -> bool:
    """What the three message kernels take: 1 .. 3 levels of 64 / 128 / 256 channels, 1 .. 8 agents, maps of fewer than 2^31 values."""
    ok = 1 <= len(channels) <= W2COMM_MAX_LEVELS and all(int(c) in (64, 128, 256) for c in channels) and 1 <= int(n_agents) <= 8
    return bool(ok and (hw is None or (len(hw) == len(channels) and all(h >= 1 and w >= 1 and c * h * w < 2 ** 31 for c, (h, w) in zip(channels, hw)))))


def w2comm_msg_index_shape_ok(n_agents: int, hw: Sequence[Tuple[int, int]]) -> bool:
    """What ``coalign_w2comm_msg_index`` takes: 1 .. 8 agents, 1 .. 3 levels of at least one pixel and fewer than 2^31."""
    return bool(1 <= int(n_agents) <= 8 and 1 <= len(hw) <= W2COMM_MAX_LEVELS and all(h >= 1 and w >= 1 and h * w < 2 ** 31 for h, w in hw))


def _words(w: int) -> int:
    return (int(w) + 31) // 32


def _ptr_array(tensors):
    return (ctypes.c_void_p * max(1, len(tensors)))(*[0 if t is None else t.data_ptr() for t in tensors])


def _i32_array(values):
    return (ctypes.c_int32 * max(1, len(values)))(*[int(v) for v in values])


@_device_op
def w2comm_msg_index(masks: Optional[Sequence[torch.Tensor]], bits: Optional[Sequence[torch.Tensor]] = None, hw: Optional[Sequence[Tuple[int, int]]] = None):
    """Bitmaps, rank tables and counts of n agents at every level in one launch (``coalign_w2comm_msg_index``).  Sender form: ``masks[l]`` [n, H_l, W_l] uint8
    (nonzero = set).  Receiver form: ``masks`` None, ``bits[l]`` [n, H_l, ceil(W_l / 32)] int32 (the words' bit patterns) and ``hw`` [(H_l, W_l)].
    -> (bits per level [n, H_l, Wd_l] int32, rank per level [n, H_l, Wd_l] int32, count [n, levels] int32)."""
    given = masks if masks is not None else bits
    if given is None or len(given) < 1:
        raise ValueError("w2comm_msg_index: masks (sender) or bits and hw (receiver)")
    _need_gpu(*given)
    n, dev = int(given[0].shape[0]), given[0].device
    if masks is not None:
        if any(m.dtype != torch.uint8 or m.dim() != 3 or m.shape[0] != n or m.device != dev for m in masks):
            raise ValueError("w2comm_msg_index: one uint8 mask [n, H, W] per level, on one device")
        masks = [m.contiguous() for m in masks]
        hw = [(int(m.shape[1]), int(m.shape[2])) for m in masks]
        bits = [torch.empty((n, h, _words(w)), dtype=torch.int32, device=dev) for h, w in hw]
    else:
        if hw is None or len(hw) != len(bits) or any(b.dtype != torch.int32 or tuple(b.shape) != (n, h, _words(w)) or b.device != dev or not b.is_contiguous() for b, (h, w) in zip(bits, hw)):
            raise ValueError("w2comm_msg_index: contiguous int32 bits [n, H, ceil(W / 32)] per level and their (H, W)")
        bits = list(bits)
    if not w2comm_msg_index_shape_ok(n, hw):
        raise ValueError("w2comm_msg_index: 1 .. 8 agents, 1 .. 3 levels")
    levels = len(hw)
    rank = [torch.empty_like(b) for b in bits]
    count = torch.empty((n, levels), dtype=torch.int32, device=dev)
    with _Timed("w2comm_msg_index"):
        hip.check(hip.lib().coalign_w2comm_msg_index(n, levels, _i32_array([h for h, _ in hw]), _i32_array([w for _, w in hw]), None if masks is None else _ptr_array(masks),
                                                     _ptr_array(bits), _ptr_array(rank), _ptr(count), _stream()), "coalign_w2comm_msg_index")
    return bits, rank, count


@_device_op
def w2comm_msg_pack(xs: Sequence[torch.Tensor], bits: Sequence[torch.Tensor], rank: Sequence[torch.Tensor], rows: Optional[Sequence[torch.Tensor]] = None) -> list:
    """Every set pixel's channel vector to its row, all agents and levels in one launch (``coalign_w2comm_msg_pack``): ``xs[l]`` [n, C_l, H_l, W_l] channels-last
    float32, ``bits`` / ``rank`` as ``w2comm_msg_index`` gives them -> rows per level [n, max(1, H_l W_l), C_l] float32 (``rows``: buffers to write into; rows
    behind an agent's count are not touched)."""
    _need_gpu(*xs, *bits, *rank)
    levels, n = len(xs), int(xs[0].shape[0])
    if not 1 <= levels <= 3 or len(bits) != levels or len(rank) != levels or any(not warp_fuse_nhwc_ok(x) or x.shape[0] != n for x in xs):
        raise ValueError("w2comm_msg_pack needs 1-3 channels-last float32 maps [n <= 8, C in {64, 128, 256}, H, W]")
    for x, b, r in zip(xs, bits, rank):
        want = (n, x.shape[2], _words(x.shape[3]))
        if any(t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous() or t.device != x.device for t in (b, r)):
            raise ValueError("w2comm_msg_pack: contiguous int32 bits and rank [n, H, ceil(W / 32)] per level, on the map's device")
    shapes = [(n, max(1, x.shape[2] * x.shape[3]), x.shape[1]) for x in xs]
    if rows is None:
        rows = [torch.empty(s, dtype=torch.float32, device=xs[0].device) for s in shapes]
    elif len(rows) != levels or any(r.dtype != torch.float32 or tuple(r.shape) != s or not r.is_contiguous() or r.device != xs[0].device for r, s in zip(rows, shapes)):
        raise ValueError("w2comm_msg_pack: rows [n, max(1, H W), C] float32 contiguous per level")
    with _Timed("w2comm_msg_pack"):
        hip.check(hip.lib().coalign_w2comm_msg_pack(n, levels, _ptr_array(xs), _i32_array([x.shape[1] for x in xs]), _i32_array([x.shape[2] for x in xs]),
                                                    _i32_array([x.shape[3] for x in xs]), _ptr_array(bits), _ptr_array(rank), _ptr_array(rows), _stream()),
                  "coalign_w2comm_msg_pack")
    return list(rows)


def _hwc_plane(t: torch.Tensor, C: int, H: int, W: int) -> bool:
    """One agent's map in (H, W, C) memory: [C, H, W] or [1, C, H, W] of a channels-last tensor."""
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    return t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (C, H, W) and (t.permute(1, 2, 0).is_contiguous())


@_device_op
def w2comm_fuse_packed(sources: Sequence[Sequence[tuple]], shapes: Sequence[Tuple[int, int, int]], theta: torch.Tensor, mode: int) -> list:
    """``w2comm_fuse_nhwc`` of ONE frame with a source per agent and scale (``coalign_w2comm_fuse_packed``).  ``shapes[i]`` = (C_i, H_i, W_i); ``sources[i][j]``
    describes agent j at scale i: ``(x, mask)`` -- a dense plane, [C, H, W] or [1, C, H, W] in (H, W, C) memory, with its uint8 mask [H, W] or None (all ones) --
    or ``(rows, bits, rank)`` -- a message's level: rows [>= 1, C] float32, bits and rank [H, ceil(W / 32)] int32.  theta [n, 2, 3] f64, mode FUSE_ATT / FUSE_MAX
    -> per scale [1, C_i, H_i, W_i] channels-last."""
    k = len(sources)
    n = len(sources[0]) if k else 0
    flat = [t for level in sources for s in level for t in s if t is not None]
    _need_gpu(*flat, theta)
    if not 1 <= k <= 3 or len(shapes) != k or not 1 <= n <= 8 or any(len(level) != n for level in sources) or any(int(C) not in (64, 128, 256) for C, _, _ in shapes):
        raise ValueError("w2comm_fuse_packed needs 1-3 scales of C in {64, 128, 256} with one source per agent (1 .. 8) each")
    if mode not in (FUSE_ATT, FUSE_MAX):
        raise ValueError("w2comm_fuse_packed fuses (FUSE_ATT | FUSE_MAX)")
    dev = flat[0].device
    kind, src, aux, rank = [], [], [], []
    for (C, H, W), level in zip(shapes, sources):
        for s in level:
            if len(s) == 2:
                x, m = s
                if not _hwc_plane(x, C, H, W) or (m is not None and (m.dtype != torch.uint8 or tuple(m.shape[-2:]) != (H, W) or m.numel() != H * W or not m.is_contiguous() or m.device != dev)):
                    raise ValueError("w2comm_fuse_packed: a dense source is (a float32 plane in (H, W, C) memory, its contiguous uint8 mask [H, W] or None)")
                kind.append(W2COMM_SRC_DENSE); src.append(x); aux.append(m); rank.append(None)
            else:
                r, b, rk = s
                ok = r.dtype == torch.float32 and r.dim() == 2 and r.shape[0] >= max(1, H * W) and r.shape[1] == C and r.is_contiguous()
                ok = ok and all(t.dtype == torch.int32 and tuple(t.shape) == (H, _words(W)) and t.is_contiguous() for t in (b, rk))
                if not ok:
                    raise ValueError("w2comm_fuse_packed: a packed source is (rows [max(1, H W), C] float32, bits [H, ceil(W / 32)] int32, rank likewise), contiguous")
                kind.append(W2COMM_SRC_PACKED); src.append(r); aux.append(b); rank.append(rk)
    th = theta.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(th.shape) != (n, 2, 3):
        raise ValueError("one theta row per agent")
    outs = [torch.empty((1, C, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last) for C, H, W in shapes]
    with _Timed("w2comm_fuse_packed"):
        hip.check(hip.lib().coalign_w2comm_fuse_packed(k, _i32_array([s[0] for s in shapes]), _i32_array([s[1] for s in shapes]), _i32_array([s[2] for s in shapes]),
                                                       _i32_array(kind), _ptr_array(src), _ptr_array(aux), _ptr_array(rank), _ptr_array(outs),
                                                       _i32_array([s[1] for s in shapes]), _i32_array([s[2] for s in shapes]), n, _ptr(th), mode, _stream()),
                  "coalign_w2comm_fuse_packed")
    return outs


# ---- Lift-Splat's frustum pooling for the camera model (include/coalign_amd_lss.h, csrc/lss_pool.hip) --------------------------------------------------------------
LSS_CHUNK = 512               # COALIGN_LSS_CHUNK
LSS_MAX_DEPTH = 128           # COALIGN_LSS_MAX_DEPTH


def lss_shape_ok(C: int, D: int) -> bool:
    """The shapes ``coalign_lss_pool`` takes: C = 64 or 128 feature channels, 1 <= D <= 128 depth bins (any number of agents, cameras, pixels and cells)."""
    return C in (64, 128) and 1 <= D <= LSS_MAX_DEPTH


class LiftSplatIndex:
    """The inverted index of one camera rig (the header's description): per output cell -- key ((a ny + y) nx + x) nz + z -- the list of its frustum points in
    ascending point order.  ``starts`` [cells + 1], ``points`` [n_points, 2] = (feature row, probability index), ``long_cells`` (lists longer than ``LSS_CHUNK``),
    all int32; ``order`` [n_points] int64, the flat point numbers in list order (what ``points`` was made of; the tests read it).  ``dims`` = (A, N, D, fH, fW,
    nx, ny, nz)."""

    def __init__(self, starts, points, long_cells, order, dims):
        self.starts, self.points, self.long_cells, self.order, self.dims = starts, points, long_cells, order, tuple(int(v) for v in dims)

    @property
    def cells(self) -> int:
        A, _, _, _, _, nx, ny, nz = self.dims
        return A * nx * ny * nz

    @property
    def n_points(self) -> int:
        return int(self.points.shape[0])

    def chunks(self):
        """[(key, begin, end)] of the pieces ``coalign_lss_pool`` sums on their own, in the order it adds them: a list of at most ``LSS_CHUNK`` points is one piece,
        a longer one is cut every ``LSS_CHUNK`` points (host lists; the tests' view of the split rule)."""
        s = self.starts.tolist()
        out = []
        for k in range(len(s) - 1):
            for b in range(s[k], s[k + 1], LSS_CHUNK):
                out.append((k, b, min(s[k + 1], b + LSS_CHUNK)))
        return out


def build_lss_index(cell: torch.Tensor, A: int, N: int, nx: int, ny: int, nz: int) -> LiftSplatIndex:
    """``cell`` [A N, D, fH, fW] int32 (``lss_cells``: (z ny + y) nx + x, or -1) -> the index, with torch ops on ``cell``'s device (CPU or GPU): a STABLE sort of the
    kept points' keys keeps every list in ascending point order, ``bincount`` / ``cumsum`` give the list starts.  Once per rig, off the frame path; it synchronises."""
    M, D, fH, fW = (int(v) for v in cell.shape)
    if M != A * N:
        raise ValueError("build_lss_index: cell must be [A N, D, fH, fW]")
    cells = A * nx * ny * nz
    if cell.numel() >= 2 ** 31 or cells >= 2 ** 31 or M * fH * fW * D >= 2 ** 31:
        raise ValueError("build_lss_index: outside int32 indexing")
    flat = cell.reshape(-1).long()
    pid = torch.arange(flat.numel(), device=cell.device)
    kept = flat >= 0
    flat, pid = flat[kept], pid[kept]
    agent = pid // (N * D * fH * fW)
    x, y, z = flat % nx, (flat // nx) % ny, flat // (nx * ny)
    key = ((agent * ny + y) * nx + x) * nz + z
    key, perm = torch.sort(key, stable=True)
    order = pid[perm]
    counts = torch.bincount(key, minlength=cells)
    starts = torch.zeros(cells + 1, dtype=torch.int64, device=cell.device)
    starts[1:] = torch.cumsum(counts, 0)
    m, rem = order // (D * fH * fW), order % (D * fH * fW)
    row = m * (fH * fW) + rem % (fH * fW)
    points = torch.stack([row, row * D + rem // (fH * fW)], dim=1).to(torch.int32).contiguous()
    long_cells = torch.nonzero(counts > LSS_CHUNK).reshape(-1).to(torch.int32).contiguous()
    return LiftSplatIndex(starts.to(torch.int32).contiguous(), points, long_cells, order, (A, N, D, fH, fW, nx, ny, nz))


@_device_op
def lss_cells(rots: torch.Tensor, trans: torch.Tensor, intrins: torch.Tensor, post_rots: torch.Tensor, post_trans: torch.Tensor, xs: torch.Tensor,
              ys: torch.Tensor, ds: torch.Tensor, lower: Sequence[float], dx: Sequence[float], n: Sequence[int], cams_per_agent: int) -> torch.Tensor:
    """The voxel of every frustum point (``coalign_lss_cells``): camera tensors [A N, 3, 3] / [A N, 3] (or the reference's [A, N, ...]) float32, the frustum's axes
    xs [fW], ys [fH], ds [D] float32, ``lower`` = bx - dx / 2 and ``dx`` as float32 values per axis, ``n`` = (nx, ny, nz) -> int32 [A N, D, fH, fW]."""
    _need_gpu(rots, trans, intrins, post_rots, post_trans, xs, ys, ds)
    r, k, pr = (_f32c(t.reshape(-1, 3, 3)) for t in (rots, intrins, post_rots))
    t, pt = (_f32c(v.reshape(-1, 3)) for v in (trans, post_trans))
    M, N = int(r.shape[0]), int(cams_per_agent)
    if N < 1 or M < 1 or M % N or any(int(v.shape[0]) != M for v in (k, pr, t, pt)):
        raise ValueError("lss_cells: five camera tensors of A N cameras each")
    xs, ys, ds = (_f32c(v.reshape(-1)).to(r.device) for v in (xs, ys, ds))
    D, fH, fW = int(ds.numel()), int(ys.numel()), int(xs.numel())
    cell = torch.empty((M, D, fH, fW), dtype=torch.int32, device=r.device)
    hip.check(hip.lib().coalign_lss_cells(_ptr(r), _ptr(t), _ptr(k), _ptr(pr), _ptr(pt), M // N, N, _ptr(xs), _ptr(ys), _ptr(ds), D, fH, fW, float(lower[0]), float(lower[1]),
                                          float(lower[2]), float(dx[0]), float(dx[1]), float(dx[2]), int(n[0]), int(n[1]), int(n[2]), _ptr(cell), _stream()), "coalign_lss_cells")
    return cell


@_device_op
def lss_depth_prob(depth_logit: torch.Tensor) -> torch.Tensor:
    """softmax over the depth bins (``coalign_lss_depth_prob``): [M, D, fH, fW] float32, plain or channels-last memory, read in place -> [M fH fW, D]."""
    _need_gpu(depth_logit)
    if depth_logit.dim() != 4 or depth_logit.dtype != torch.float32:
        raise ValueError("lss_depth_prob needs float32 logits [M, D, fH, fW]")
    M, D, fH, fW = (int(v) for v in depth_logit.shape)
    nhwc = depth_logit.permute(0, 2, 3, 1).is_contiguous()
    x = depth_logit if nhwc or depth_logit.is_contiguous() else depth_logit.contiguous()
    prob = torch.empty((M * fH * fW, D), dtype=torch.float32, device=x.device)
    with _Timed("lss_depth_prob"):
        hip.check(hip.lib().coalign_lss_depth_prob(_ptr(x), M, D, fH, fW, int(nhwc and not x.is_contiguous()), _ptr(prob), _stream()), "coalign_lss_depth_prob")
    return prob


@_device_op
def lss_pool(depth_logit: torch.Tensor, x_img: torch.Tensor, index: LiftSplatIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The frame path of the frustum pooling, two launches (``coalign_lss_depth_prob``, ``coalign_lss_pool``): depth_logit [A N, D, fH, fW], x_img [A N, C, fH, fW]
    float32 -> the BEV map [A, nz C, ny, nx] (channel z C + c) in channels-last memory, every element written.  ``x_img`` is read in place when it is channels-last
    (a point's C values are one row); a plain NCHW map is brought into that layout by torch first.  ``out``: a channels-last buffer to write into."""
    _need_gpu(depth_logit, x_img, index.points)
    A, N, D, fH, fW, nx, ny, nz = index.dims
    if x_img.dim() != 4 or x_img.dtype != torch.float32 or tuple(depth_logit.shape) != (A * N, D, fH, fW) or (x_img.shape[0], x_img.shape[2], x_img.shape[3]) != (A * N, fH, fW):
        raise ValueError("lss_pool: depth_logit [A N, D, fH, fW] and x_img [A N, C, fH, fW] float32 of the index's camera rig")
    C = int(x_img.shape[1])
    if not lss_shape_ok(C, D):
        raise hip.CoalignHipError("lss_pool: C in {64, 128} and 1 <= D <= 128")
    rows = x_img.permute(0, 2, 3, 1)
    if not rows.is_contiguous():
        rows = rows.contiguous()
    prob = lss_depth_prob(depth_logit)
    if out is None:
        out = torch.empty((A, ny, nx, nz * C), dtype=torch.float32, device=rows.device).permute(0, 3, 1, 2)
    elif tuple(out.shape) != (A, nz * C, ny, nx) or out.dtype != torch.float32 or not out.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError("lss_pool: out must be a channels-last float32 map [A, nz C, ny, nx]")
    with _Timed("lss_pool"):
        hip.check(hip.lib().coalign_lss_pool(_ptr(rows), _ptr(prob), A * N * fH * fW, C, D, _ptr(index.points), index.n_points, _ptr(index.starts), index.cells,
                                             _ptr(index.long_cells), int(index.long_cells.numel()), _ptr(out), _stream()), "coalign_lss_pool")
    return out


# ---- the camera model's BEV encoder (include/coalign_amd_lss_bev.h, csrc/lss_bev.hip) ---------------------------------------------------------------------------
CONV7X7_COUT = 64             # COALIGN_CONV7X7_COUT
CONV7X7_MAX_CIN = 512         # COALIGN_CONV7X7_MAX_CIN


def conv7x7_s2_shape_ok(cin: int, cout: int = CONV7X7_COUT) -> bool:
    """A 7 x 7 / stride-2 layer of (cin, cout) fits ``coalign_conv7x7_s2_sp``."""
    return cout == CONV7X7_COUT and cin % 16 == 0 and 16 <= cin <= CONV7X7_MAX_CIN


def pack_conv7x7_s2_weight(weight: torch.Tensor) -> torch.Tensor:
    """[64, Cin, 7, 7] fp32 (Cin % 16 == 0, 16 <= Cin <= 512) -> the weight image of ``coalign_conv7x7_s2_sp`` as uint8 (include/coalign_amd_lss_bev.h (18a)):
    [Cin / 16][7 ky][7 kx][2 terms][2 channel halves][64 cout][8 cin] fp16 sp16 pairs of the per-output-channel scaled weights (the scaling and rounding of
    ``pack_conv3x3_emu_weight``'s terms-16 image), 16 zero bytes, [64] float32 2^-k_c, [64] float32 2^k_c."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) != (7, 7) or not conv7x7_s2_shape_ok(ci, co):
        raise ValueError(f"conv7x7_s2_sp needs 7x7 weights with Cout == {CONV7X7_COUT}, Cin % 16 == 0 and 16 <= Cin <= {CONV7X7_MAX_CIN}, got {tuple(weight.shape)}")
    wf = weight.detach().float()
    w = wf.reshape(co, ci // 16, 2, 8, 7, 7).permute(1, 4, 5, 2, 0, 3)    # [interval, ky, kx, channel half, cout, cin]
    amax = wf.abs().reshape(co, -1).amax(dim=1)
    k = torch.where(amax > 0, 14 - torch.frexp(amax)[1], torch.zeros_like(amax, dtype=torch.int32)).clamp(-60, 60).to(torch.int32)
    scale = torch.ldexp(torch.ones_like(amax), k)
    ws = (w * scale.reshape(1, 1, 1, 1, co, 1)).contiguous()
    ws = ((ws.view(torch.int32) + 2) & -4).view(torch.float32)             # 22 significant bits, ties away from zero (sp16_round)
    hi = ws.half()
    lo = ((ws - hi.float()) * 1024.0).half()
    flat = torch.stack([hi, lo], dim=3).contiguous().view(torch.uint8).reshape(-1)      # [interval, ky, kx, term, channel half, cout, cin]
    tail = [torch.ldexp(torch.ones_like(amax), -k).contiguous().view(torch.uint8).reshape(-1), scale.contiguous().view(torch.uint8).reshape(-1)]
    out = torch.cat([flat, torch.zeros(16, dtype=torch.uint8, device=flat.device)] + tail)
    assert out.numel() == hip.lib().coalign_conv7x7_s2_weight_bytes(ci)
    return out


@_device_op
def conv7x7_s2_sp(x: torch.Tensor, image: torch.Tensor, bias: torch.Tensor, relu: bool = True) -> "SplitMap":
    """y = act(conv7x7(x, w, stride 2, padding 3) + bias) with 64 output channels, written as a ``SplitMap`` (include/coalign_amd_lss_bev.h (18b)): the stem of
    ``lss.BevEncodeMSFusion``.  ``x``: float32 of logical shape [N, C, H, W], read in place when its memory is channels-last (what ``lss_pool`` writes), converted
    by torch first when it is NCHW; ``image``: ``pack_conv7x7_s2_weight``; ``bias`` [64]."""
    _need_gpu(x, image, bias)
    if x.dim() != 4:
        raise ValueError("conv7x7_s2_sp reads a [N, C, H, W] tensor")
    N, Cin, H, W = (int(v) for v in x.shape)
    L = hip.lib()
    if not conv7x7_s2_shape_ok(Cin) or image.numel() != L.coalign_conv7x7_s2_weight_bytes(Cin) or bias.numel() != CONV7X7_COUT:
        raise ValueError(f"conv7x7_s2_sp needs Cin % 16 == 0, 16 <= Cin <= {CONV7X7_MAX_CIN}, the weight image of Cin and {CONV7X7_COUT} biases")
    if H < 1 or W < 1:
        raise ValueError("conv7x7_s2_sp needs H, W >= 1")
    xt = to_nhwc(x)
    out = SplitMap.empty(N, CONV7X7_COUT, (H - 1) // 2 + 1, (W - 1) // 2 + 1, xt.device)
    with _Timed("conv7x7_s2_sp"):
        hip.check(L.coalign_conv7x7_s2_sp(_ptr(xt), _ptr(image), _ptr(_f32c(bias)), _ptr(out.data), N, Cin, H, W, int(bool(relu)), _ptr(sp_range_flag(xt.device)), _stream()),
                  "coalign_conv7x7_s2_sp")
    return out


@_device_op
def up2x_concat_sp(skip: torch.Tensor, low: torch.Tensor) -> "SplitMap":
    """SplitMap of ``cat([skip, up(low)], dim=1)``, ``up`` = bilinear x 2 with ``align_corners=True``, in one pass (include/coalign_amd_lss_bev.h (18c)): ``lss.Up``
    up to its convolutions.  ``skip`` [N, Cs, 2h, 2w], ``low`` [N, Cl, h, w], float32, read in place when channels-last, converted by torch first when NCHW."""
    _need_gpu(skip, low)
    if skip.dim() != 4 or low.dim() != 4:
        raise ValueError("up2x_concat_sp reads two [N, C, H, W] tensors")
    N, Cs, H2, W2 = (int(v) for v in skip.shape)
    Nl, Cl, h, w = (int(v) for v in low.shape)
    if Nl != N or (H2, W2) != (2 * h, 2 * w) or h < 1 or w < 1:
        raise ValueError(f"up2x_concat_sp: skip {tuple(skip.shape)} must be [N, Cs, 2h, 2w] for low {tuple(low.shape)} = [N, Cl, h, w]")
    if Cs % 16 or Cl % 16 or Cs < 16 or Cl < 16:
        raise ValueError("up2x_concat_sp needs Cs % 16 == 0 and Cl % 16 == 0")
    st, lt = to_nhwc(skip), to_nhwc(low)
    out = SplitMap.empty(N, Cs + Cl, H2, W2, st.device)
    with _Timed("up2x_concat_sp"):
        hip.check(hip.lib().coalign_up2x_concat_sp(_ptr(st), _ptr(lt), _ptr(out.data), N, Cs, Cl, h, w, _ptr(sp_range_flag(st.device)), _stream()), "coalign_up2x_concat_sp")
    return out


# ---- the SSFA neck of the SECOND detectors (include_open/coalign_amd_ssfa.h, csrc/ssfa_neck.hip) -----------------------------------------------------------
DECONV3X3_MAX_COUT = 1024     # COALIGN_DECONV3X3_MAX_COUT
DECONV3X3_TILE = (8, 16)      # COALIGN_DECONV3X3_TILE_H, COALIGN_DECONV3X3_TILE_W: input pixels of a workgroup
SSFA_BLEND_MAX_C = 512        # COALIGN_SSFA_BLEND_MAX_C


def deconv3x3_s2_shape_ok(cin: int, cout: int) -> bool:
    """A ConvTranspose2d 3 x 3 / stride-2 layer of (cin, cout) fits ``coalign_deconv3x3_s2_sp``."""
    return cin % 16 == 0 and cin >= 16 and cout % 64 == 0 and 64 <= cout <= DECONV3X3_MAX_COUT


@_device_op
def deconv3x3_s2_sp(x: "SplitMap", w_image: torch.Tensor, bias: torch.Tensor, cout: int, residual: Optional[torch.Tensor] = None, relu: bool = True) -> "SplitMap":
    """y = act(conv_transpose3x3(x, w, stride 2, padding 1, output_padding 1) + bias) (+ ``residual``, AFTER the activation) on SplitMaps
    (include_open/coalign_amd_ssfa.h (19b)).  ``w_image``: ``pack_conv3x3_emu_weight(w.permute(1, 0, 2, 3), 16, True)`` of the ConvTranspose2d weight
    [Cin, Cout, 3, 3]; ``residual``: float32 of logical shape [N, Cout, 2h, 2w] (converted to channels-last memory if it is not) or None."""
    if not isinstance(x, SplitMap):
        raise TypeError("deconv3x3_s2_sp reads a SplitMap")
    _need_gpu(x.data, w_image, bias)
    L = hip.lib()
    N, Cin, h, w = x.shape
    if not deconv3x3_s2_shape_ok(Cin, cout) or w_image.numel() != L.coalign_deconv3x3_s2_weight_bytes(Cin, cout) or bias.numel() != cout:
        raise ValueError("deconv3x3_s2_sp needs Cin % 16 == 0, Cout % 64 == 0, the tap-major terms-16 weight image of (Cin, Cout) and Cout biases")
    res_t = None
    if residual is not None:
        res_t = to_nhwc(residual)
        if tuple(res_t.shape) != (N, cout, 2 * h, 2 * w):
            raise ValueError("residual shape mismatch")
    out = SplitMap.empty(N, cout, 2 * h, 2 * w, x.device)
    with _Timed("deconv3x3_s2_sp"):
        hip.check(L.coalign_deconv3x3_s2_sp(_ptr(x.data), _ptr(w_image), _ptr(_f32c(bias)), _ptr(res_t), _ptr(out.data), N, Cin, cout, h, w, int(bool(relu)),
                                            _ptr(sp_range_flag(x.device)), _stream()), "coalign_deconv3x3_s2_sp")
    return out


@_device_op
def ssfa_blend(a: torch.Tensor, b: torch.Tensor, wa: torch.Tensor, wb: torch.Tensor, ba: float, bb: float, out_split: bool = False, out_nhwc: bool = True):
    """p = softmax over (wa . a + ba, wb . b + bb) per pixel, y = a p + b (1 - p) in one launch (include_open/coalign_amd_ssfa.h (19c)).  ``a``, ``b``: float32 of
    logical shape [N, C, H, W] (read in place when channels-last); ``wa``, ``wb`` [C].  Returns the channels-last float32 tensor (``out_nhwc``), the SplitMap of it
    (``out_split``), or the pair (tensor, SplitMap) when both are asked for."""
    _need_gpu(a, b, wa, wb)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError("ssfa_blend reads two [N, C, H, W] tensors of one shape")
    if not (out_split or out_nhwc):
        raise ValueError("ssfa_blend: at least one output")
    N, C, H, W = (int(v) for v in a.shape)
    if C % 16 or not 16 <= C <= SSFA_BLEND_MAX_C or wa.numel() != C or wb.numel() != C:
        raise ValueError(f"ssfa_blend needs C % 16 == 0, 16 <= C <= {SSFA_BLEND_MAX_C} and [C] weights")
    at, bt = to_nhwc(a), to_nhwc(b)
    y = ysp = None
    if out_nhwc:
        y = torch.empty((N, H, W, C), dtype=torch.float32, device=at.device).permute(0, 3, 1, 2)
    if out_split:
        ysp = SplitMap.empty(N, C, H, W, at.device)
    with _Timed("ssfa_blend"):
        hip.check(hip.lib().coalign_ssfa_blend(_ptr(at), _ptr(bt), _ptr(_f32c(wa).reshape(-1)), _ptr(_f32c(wb).reshape(-1)), float(ba), float(bb), _ptr(y),
                                               _ptr(None if ysp is None else ysp.data), N, C, H, W, _ptr(sp_range_flag(at.device)) if out_split else None, _stream()),
                  "coalign_ssfa_blend")
    return (y, ysp) if (out_split and out_nhwc) else (ysp if out_split else y)


# ---- the sparse 3-D trunk of the SECOND detectors (include_ext/coalign_amd_sparse3d.h, csrc/sparse_conv3d.hip) -----------------------------------------------
SP3D_COMBINATIONS = {27: ((4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64)), 3: ((64, 64), (64, 128))}
SP3D_STATUS_OVERFLOW = 1


def sp3d_supported(cin: int, cout: int, taps: int) -> bool:
    """The (Cin, Cout, taps) combinations ``coalign_sp3d_conv`` takes: VoxelBackBone8x's own."""
    return (cin, cout) in SP3D_COMBINATIONS.get(taps, ())


def pack_sp3d_weights(w: torch.Tensor) -> torch.Tensor:
    """Folded weights [Cout, taps, Cin] float32 -> the image of ``coalign_sp3d_conv`` (header (18f)): float32 [taps][Cin][Cout] at Cin = 4, else the sp16 operand image
    of [Cout rounded up to 32, taps Cin] (``_disco_operand_image``: column k = tap Cin + c, rows past Cout zero) with every row DIVIDED by a power of two 2^k_c that
    brings its largest |w| into [1, 2) (a zero row: k_c = 0), followed by the float32 values 2^k_c, one per row.  An unscaled pair keeps an absolute 2^-34 of a weight
    below 2^-14, so a channel whose folded batch-norm scale is small would lose most of its digits; the division is exact and the kernel multiplies it back."""
    cout, taps, cin = w.shape
    w = w.detach().float()
    if cin == 4:
        return w.permute(1, 2, 0).contiguous().view(torch.uint8).reshape(-1)
    rows = (cout + 31) // 32 * 32
    flat = w.reshape(cout, taps * cin)
    top = flat.abs().amax(dim=1)
    k = ((top.contiguous().view(torch.int32) >> 23) & 0xFF) - 127                              # floor(log2) of a normal value, from its exponent field
    k = torch.where((top > 0) & torch.isfinite(top), k.clamp(-126, 126), torch.zeros_like(k))
    full = w.new_zeros((rows, taps * cin))
    full[:cout] = flat * ((127 - k) << 23).view(torch.float32).view(-1, 1)                     # x 2^-k, exact
    tail = w.new_ones(rows)
    tail[:cout] = ((127 + k) << 23).view(torch.float32)
    return torch.cat([_disco_operand_image(full), tail.contiguous().view(torch.uint8)]).contiguous()


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _triple(v) -> Tuple[int, int, int]:
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(a) for a in v)


def sp3d_out_shape(shape, k, s, p) -> Tuple[int, int, int]:
    """spconv's output shape per axis: (n + 2 p - k) // s + 1."""
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(shape, _triple(k), _triple(s), _triple(p)))


@_device_op
def sp3d_mean_vfe(voxels: torch.Tensor, num_points: torch.Tensor) -> torch.Tensor:
    """MeanVFE: voxels [M, T, C] float32, num_points [M] -> [M, C] (one launch)."""
    _need_gpu(voxels, num_points)
    M, T, C = voxels.shape
    voxels, n = _f32c(voxels), num_points.to(torch.int32).contiguous()
    out = torch.empty((M, C), dtype=torch.float32, device=voxels.device)
    with _Timed("sp3d_mean_vfe"):
        hip.check(hip.lib().coalign_sp3d_mean_vfe(_ptr(voxels), _ptr(n), M, T, C, _ptr(out), _stream()), "coalign_sp3d_mean_vfe")
    return out


def sp3d_index_bytes(batch: int, shape, capacity: int) -> int:
    n = hip.lib().coalign_sp3d_index_workspace_bytes(batch, *shape, capacity)
    if n == 0:
        raise ValueError(f"sparse grid {batch} x {tuple(shape)} is outside the kernels' range (N D H W < 2^31)")
    return n


@_device_op
def sp3d_index_build(indices: torch.Tensor, count: torch.Tensor, batch: int, shape) -> torch.Tensor:
    """The site index (bitmap + word prefix + rank -> row) of ``indices`` [capacity, 4] int32 with its device ``count``; a uint8 tensor.  Six launches, no read-back."""
    _need_gpu(indices, count)
    cap = indices.shape[0]
    nbytes = sp3d_index_bytes(batch, shape, cap)
    index = torch.empty(nbytes, dtype=torch.uint8, device=indices.device)
    with _Timed("sp3d_index"):
        hip.check(hip.lib().coalign_sp3d_index_build(_ptr(indices), _ptr(count), cap, batch, *shape, _ptr(index), nbytes, _stream()), "coalign_sp3d_index_build")
    return index


@_device_op
def sp3d_strided_sites(indices: torch.Tensor, count: torch.Tensor, batch: int, shape, k, s, p, cap_out: int, status: torch.Tensor):
    """Output sites of a strided sparse convolution, ascending in the cell index: (out_indices [cap_out, 4], out_count [1] on the device, out_index).  Six launches."""
    _need_gpu(indices, count, status)
    k, s, p = _triple(k), _triple(s), _triple(p)
    oshape = sp3d_out_shape(shape, k, s, p)
    nbytes = sp3d_index_bytes(batch, oshape, cap_out)
    dev = indices.device
    out_indices = torch.empty((cap_out, 4), dtype=torch.int32, device=dev)
    out_count = torch.empty(1, dtype=torch.int32, device=dev)
    index = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _Timed("sp3d_sites"):
        hip.check(hip.lib().coalign_sp3d_strided_sites(_ptr(indices), _ptr(count), indices.shape[0], batch, *shape, *k, *s, *p, _ptr(out_indices), _ptr(out_count), cap_out,
                                                       _ptr(index), nbytes, _ptr(status), _stream()), "coalign_sp3d_strided_sites")
    return out_indices, out_count, index


@_device_op
def sp3d_neighbors(out_indices: torch.Tensor, out_count: torch.Tensor, batch: int, out_shape, in_index: torch.Tensor, cap_in: int, in_shape, k, s, p) -> torch.Tensor:
    """The neighbour table [taps, cap_out] int32 of the output rows against the indexed input tensor (one launch)."""
    _need_gpu(out_indices, out_count, in_index)
    k, s, p = _triple(k), _triple(s), _triple(p)
    cap_out = out_indices.shape[0]
    nbr = torch.empty((k[0] * k[1] * k[2], cap_out), dtype=torch.int32, device=out_indices.device)
    with _Timed("sp3d_neighbors"):
        hip.check(hip.lib().coalign_sp3d_neighbors(_ptr(out_indices), _ptr(out_count), cap_out, batch, *out_shape, _ptr(in_index), in_index.numel(), cap_in, *in_shape,
                                                   *k, *s, *p, _ptr(nbr), _stream()), "coalign_sp3d_neighbors")
    return nbr


@_device_op
def sp3d_conv(in_feat: torch.Tensor, nbr: torch.Tensor, out_count: torch.Tensor, cout: int, weights: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """relu(sum over the taps of W[tap] in[nbr[tap]] + shift) for the rows below the device count -> [cap_out, Cout] (rows past the count are not written)."""
    _need_gpu(in_feat, nbr, out_count, weights, shift)
    cap_in, cin = in_feat.shape
    taps, cap_out = nbr.shape
    out = torch.empty((cap_out, cout), dtype=torch.float32, device=in_feat.device)
    with _Timed("sp3d_conv"):
        hip.check(hip.lib().coalign_sp3d_conv(_ptr(in_feat), cap_in, _ptr(nbr), taps, _ptr(out_count), cap_out, cin, cout, _ptr(weights), weights.numel(), _ptr(shift),
                                              _ptr(out), _stream()), "coalign_sp3d_conv")
    return out


@_device_op
def sp3d_to_dense(feat: torch.Tensor, count: torch.Tensor, index: torch.Tensor, batch: int, shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dense() + HeightCompression's view: [N, C D, H, W] float32 in channels-last memory, channel c D + d, every element written by the launch (into ``out`` when
    given: a channels-last tensor of that shape, whatever it holds)."""
    _need_gpu(feat, count, index)
    cap, C = feat.shape
    D, H, W = shape
    if out is None:
        out = torch.empty((batch, C * D, H, W), dtype=torch.float32, device=feat.device, memory_format=torch.channels_last)
    elif tuple(out.shape) != (batch, C * D, H, W) or out.dtype != torch.float32 or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("sp3d_to_dense: out must be a channels-last float32 [N, C D, H, W] tensor")
    with _Timed("sp3d_to_dense"):
        hip.check(hip.lib().coalign_sp3d_to_dense(_ptr(feat), _ptr(count), cap, C, _ptr(index), index.numel(), batch, D, H, W, _ptr(out), _stream()), "coalign_sp3d_to_dense")
    return out


# ---- raw point clouds -> the trunk's input sparse tensor (include_open/coalign_amd_sp3d_voxelize.h, csrc/sparse_conv3d.hip) -----------------------------------
SP3D_STATUS_MAX_VOXELS = 2            # COALIGN_SP3D_STATUS_MAX_VOXELS
SP3D_VOXELIZE_MAX_POINTS = 8          # COALIGN_SP3D_VOXELIZE_MAX_POINTS
SP3D_VOXELIZE_MAX_CLOUDS = 16         # COALIGN_SP3D_VOXELIZE_MAX_CLOUDS


def sp3d_voxel_grid(voxel_size: Sequence[float], lidar_range: Sequence[float]) -> Tuple[int, int, int]:
    """The voxel grid (x, y, z) as the kernels and ``coalign_voxelize`` compute it: round((hi - lo) / vs) in float32 (sp_voxel_preprocessor.py:40-42)."""
    r, v = np.asarray(lidar_range, dtype=np.float32), np.asarray(voxel_size, dtype=np.float32)
    return tuple(int(g) for g in np.round((r[3:6] - r[0:3]) / v))


@_device_op
def sp3d_voxelize(points: torch.Tensor, offsets: torch.Tensor, voxel_size: Sequence[float], lidar_range: Sequence[float], shape, max_points: int, max_voxels: int,
                  capacity: int, ego_filter: bool = False, filter_range: Optional[Sequence[float]] = None, status: Optional[torch.Tensor] = None):
    """points [P_cap, 4] float32 (the clouds of a frame concatenated), ``offsets``: DEVICE int32 [n_clouds + 1] -> (features [capacity, 4] mean of each voxel's first
    ``max_points`` points, indices [capacity, 4] int32 (cloud, z, y, x) ascending in the linear cell index of the sparse ``shape`` (D, H, W), count [1] int32, cloud_counts
    [n_clouds + 1] int32, the site index, status [1] int32), all on the device: no host read, no synchronisation, safe inside a captured graph (the offsets are read by
    the kernels, so a replay may see other clouds of other lengths)."""
    _need_gpu(points, offsets)
    L = hip.lib()
    if points.dim() != 2 or points.shape[1] != 4 or points.dtype != torch.float32:
        raise ValueError(f"points must be float32 [P, 4], got {points.dtype} {tuple(points.shape)}")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError("offsets must be a device int32 tensor [n_clouds + 1]")
    pts, off = _aligned16(points), offsets.contiguous()
    n_clouds, P_cap = off.numel() - 1, pts.shape[0]
    D, H, W = (int(v) for v in shape)
    dev = pts.device
    vs, rg = _dbl3(voxel_size), (ctypes.c_double * 6)(*[float(v) for v in lidar_range])
    fr = None if filter_range is None else (ctypes.c_double * 6)(*[float(v) for v in filter_range])
    flags = (VOX_FILTER_EGO if ego_filter else 0) | (VOX_FILTER_RANGE if filter_range is not None else 0)
    ws_bytes = L.coalign_sp3d_voxelize_workspace_bytes(P_cap, n_clouds, int(max_points))
    if ws_bytes == 0:
        raise ValueError(f"sp3d_voxelize: {P_cap} points, {n_clouds} clouds (1 .. {SP3D_VOXELIZE_MAX_CLOUDS}), max_points {max_points} (1 .. {SP3D_VOXELIZE_MAX_POINTS}) "
                         "is outside the kernels' range")
    nbytes = sp3d_index_bytes(n_clouds, (D, H, W), capacity)
    features = torch.empty((capacity, 4), dtype=torch.float32, device=dev)
    indices = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    cloud_counts = torch.empty(n_clouds + 1, dtype=torch.int32, device=dev)
    index = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _Timed("sp3d_voxelize"):
        hip.check(L.coalign_sp3d_voxelize(_ptr(pts), _ptr(off), P_cap, n_clouds, vs, rg, D, H, W, int(max_points), int(max_voxels), flags, fr, _ptr(features), _ptr(indices),
                                          _ptr(count), _ptr(cloud_counts), int(capacity), _ptr(index), nbytes, _ptr(status), _ptr(ws), ws_bytes, _stream()),
                  "coalign_sp3d_voxelize")
    return features, indices, count, cloud_counts, index, status
