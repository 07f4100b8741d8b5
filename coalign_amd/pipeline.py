"""Frame pipeline: the reference's inference loop with several frames in flight on one GPU.

The reference runs ``for batch in loader: out = model(batch); boxes, scores = dataset.post_process(batch, out)``
strictly one frame after the other on the default stream, with a device->host synchronisation inside NMS
(opencood/tools/inference.py:125-179, inference_utils.py:122-173).  Frames are independent, so this runner keeps
``lanes`` of them in flight, each on its own HIP stream ("lane"): the partial last wave of every convolution launch
and the small latency-bound fusion / head / decode / NMS kernels of one frame overlap the other frames' work.
Results come back in submission order, ``result_lag`` frames late (the host waits for the OLDEST frame only).
``queue_depth`` (round 5) queues that many frames per stream -- ``lanes x queue_depth`` pipeline lanes, lane i on stream
i mod lanes, each with graphs and result buffers of its own --, so a stream's next frame is already enqueued when its
current one finishes: the throughput configuration is ``lanes=2, queue_depth=3, result_lag=5`` (bench.py).

Two launch modes:

* eager               ~150 host-side launches per frame through the C ABI (1.5 ms of host time); decode + NMS on a side stream.
* HIP graph (``graph=True``)  encode -> fuse -> heads -> decode -> NMS -> range filter -> the four result scalars'
  copy to pinned host memory are captured ONCE per (lane, input shape) and replayed with one host call per frame
  (every kernel has static launch geometry; data-dependent sizes live in device memory).  Round 5: a from-pillars frame is read IN PLACE -- the pillar launch
  takes its three arrays and the count through a 32-byte device record (include/coalign_amd.h (1c)) that travels, with the host-normalised pose matrices when
  the batch carries ``pairwise_t_matrix_host`` (the dataset's float64 host copy), as ONE small host-to-device transfer per frame; frames in other dtypes /
  layouts, and models whose encoder does not take a record, are copied into the graph's static buffers as before.  A new input shape triggers a new capture;
  ragged pillar counts share a capacity-sized graph per power-of-two bucket.

Both modes produce bit-identical detections to ``model(batch)`` + ``post_processor.post_process`` (tests/test_pipeline_gpu.py).

``submit_points`` is the loop as the reference runs it -- from RAW point clouds in host memory (opencood/tools/inference.py:125-130 moves
the collated batch to the device every frame, train_utils.py:249-258; the voxeliser ran in the DataLoader workers before that,
sp_voxel_preprocessor.py:62-85): host -> device copy of the frame's clouds out of a pinned staging buffer, ``coalign_voxelize``,
``coalign_pillar_encode_stream`` (the pillar count never leaves the device) and the rest of the frame, all on the lane's stream -- in graph
mode one async copy + one replay per frame.  ``latencies_ms`` records, per frame, host time from ``submit*`` to the detections in hand.

``aligner`` (``box_align.Aligner``) puts ONLINE POSE CORRECTION in front of the fusion model, inside the frame: a frame then carries ``lidar_poses`` ([N, 6]
float64: x, y, z, roll, yaw, pitch; degrees; host or device) instead of ``pairwise_t_matrix``, and its body is stage-1 forward -> ``post_process_stage1_device`` ->
``PoseCorrector.correct`` (``box_align.correct_frame_poses``, the chain ``inference_intermediate_fusion_aligned`` runs) -> the fusion model on the corrected
matrices -> post-process, all on the lane's one stream and, with ``graph``, in the lane's one captured graph.  ``alignments`` receives ``(index, status word,
corrected lidar_poses [N, 6])`` per collected frame.
"""
from __future__ import annotations

import collections
import os
import time
import weakref
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .encoder import host_ints
from .pose import normalize_pairwise_np
from .postprocess import PostProcessHandle, VoxelPostprocessor

FRAME_RECORDS = os.environ.get("COALIGN_FRAME_RECORDS", "1") != "0"            # measurement switch: 0 = every frame is copied into the graph's input buffers (rounds 2-4)

FrameResult = Tuple[int, Optional[torch.Tensor], Optional[torch.Tensor]]      # (frame index, pred_box3d [K', 8, 3], scores [K'])


def pad_pillars(processed_lidar: Dict[str, torch.Tensor], multiple: int = 4096) -> Dict[str, torch.Tensor]:
    """Pad the pillar arrays to the next multiple of ``multiple`` rows so that consecutive frames share one graph.
    Padding rows carry agent index -1: ``coalign_pillar_vfe_scatter`` ignores pillars outside the canvas / agent range."""
    vf, vc, vn = processed_lidar["voxel_features"], processed_lidar["voxel_coords"], processed_lidar["voxel_num_points"]
    m = vf.shape[0]
    target = max(multiple, (m + multiple - 1) // multiple * multiple)
    if target == m:
        return processed_lidar
    pad = target - m
    return {"voxel_features": torch.cat([vf, vf.new_zeros((pad,) + tuple(vf.shape[1:]))]),
            "voxel_coords": torch.cat([vc, vc.new_full((pad, vc.shape[1]), -1)]),
            "voxel_num_points": torch.cat([vn, vn.new_ones(pad)])}


_PILLAR_ARRAYS = ("voxel_features", "voxel_coords", "voxel_num_points")


def _pose_key(src: dict) -> str:
    """The name of a frame's small non-pillar input: the noisy ``lidar_poses`` of an aligned frame, else ``pairwise_t_matrix``."""
    return "lidar_poses" if "lidar_poses" in src else "pairwise_t_matrix"


def _points_batch(voxelizer: tuple, pts: torch.Tensor, offsets: List[int], record: List[int], pose, pose_key: str = "pairwise_t_matrix") -> dict:
    """Raw points (device) -> the model's batch, pillar count left on the device (PillarVFE's ``voxel_count_dev`` form)."""
    pre, ego_filter, filter_range = voxelizer
    voxels, coords, num, counts = ops.voxelize(pts, offsets, pre.voxel_size, pre.lidar_range, pre.max_points_per_voxel, pre.max_voxels,
                                               ego_filter=ego_filter, filter_range=filter_range)
    return {"processed_lidar": {"voxel_features": voxels, "voxel_coords": coords, "voxel_num_points": num,
                                "voxel_count_dev": counts[len(offsets) - 1:], "voxel_cells_unique": True},
            "record_len": record, pose_key: pose}


class _GraphSlot:
    """One captured frame: the graph, the decode buffers it writes, the canvas it owns.  What the frame READS is the subclass's: a constructor that allocates
    from the first frame's ``src``, ``stage(src, pose_host)`` (the per-frame host-to-device work) and ``batch(record)`` (what the model is captured on)."""
    record = affine_view = capacity = None              # fields of single forms that read as "not this form" on every slot

    def __init__(self, weights_sig):
        self.inputs: Dict[str, torch.Tensor] = {}       # static device buffers the frame is copied into
        self.buf: Optional[ops.DecodeBuffers] = None
        self.weights_sig = weights_sig
        self.canvas_cache: dict = {}
        self.canvas_cache1: dict = {}                   # the stage-1 encoder's (aligned frames)
        self.corrector = self.align_host = None         # aligned frames: the slot's PoseCorrector, and the pinned block its status word and corrected poses are copied to
        self.replays = 0                                # launches through this slot's sparse canvas since its stamps were last zeroed (ops.SPARSE_TAG_RESET_AFTER)
        # `graph`: the whole frame or, with an `exchange` (multi-rank frames), the encoder, and `tail` the ego tail: the collective runs between the two replays
        self.graph = self.tail = self.tail_record = None
        self.feats = self.affine = None                 # the encoder graph's output maps (the collective's send buffers) and pose matrices
        # the collective's output maps the tail graph was captured on: data pointers, the maps themselves (the tail graph reads them: kept referenced), row table
        self.recv_ptrs = self.recv_keep = self.rows = None


class _PointsSlot(_GraphSlot):
    """Raw points: the pinned staging buffer is copied into the static ``points`` buffer, the voxeliser runs inside the captured frame."""
    def __init__(self, weights_sig, src: dict, device, offsets: Sequence[int], voxelizer: tuple):
        super().__init__(weights_sig)
        self.offsets, self.voxelizer = list(offsets), voxelizer      # first point slot of every cloud in the static input buffer | _points_batch's settings
        self.pose_key = _pose_key(src)
        self.inputs = {name: torch.zeros(t.shape, dtype=t.dtype, device=device) for name, t in src.items()}

    def stage(self, src: dict, pose_host) -> None:
        for name, t in src.items():
            self.inputs[name].copy_(t, non_blocking=True)

    def batch(self, record: List[int]) -> dict:
        return _points_batch(self.voxelizer, self.inputs["points"], self.offsets, record, self.inputs[self.pose_key], self.pose_key)


class _PillarCopySlot(_GraphSlot):
    """Pillars copied into static buffers: at their exact shape (``capacity`` None), or into ``capacity`` rows with the frame's count on the device."""
    def __init__(self, weights_sig, src: dict, device, capacity: Optional[int]):
        super().__init__(weights_sig)
        self.capacity, self.pose_key = capacity, _pose_key(src)
        for name, t in src.items():
            rows = t.shape[0] if capacity is None or name not in _PILLAR_ARRAYS else capacity
            self.inputs[name] = torch.zeros((rows,) + t.shape[1:], dtype=t.dtype, device=device)
        if capacity is not None:
            self.count = torch.zeros(1, dtype=torch.int32, device=device)
            self.count_host = torch.zeros(1, dtype=torch.int32).pin_memory()      # (a 4-byte copy per frame, not a fill kernel)

    def stage(self, src: dict, pose_host) -> None:
        for name, t in src.items():
            dst = self.inputs[name]             # (capacity-sized buffers: the frame's rows only, rows beyond the count are never read)
            (dst if self.capacity is None or name not in _PILLAR_ARRAYS else dst[: t.shape[0]]).copy_(t, non_blocking=True)
        if self.capacity is not None:
            self.count_host[0] = int(src["voxel_features"].shape[0])
            self.count.copy_(self.count_host, non_blocking=True)

    def batch(self, record: List[int]) -> dict:
        pl = {k: self.inputs[k] for k in _PILLAR_ARRAYS}
        if self.capacity is not None:
            pl.update(voxel_count_dev=self.count, voxel_cells_unique=False)
        return {"processed_lidar": pl, "record_len": record, self.pose_key: self.inputs[self.pose_key]}


class _PillarRecordSlot(_GraphSlot):
    """Round 5: pillars read IN PLACE through a device record (ops.PillarFrameRecord), where they are (the batch stays referenced until its frame has completed):
    ``blob`` = record words (array pointers | pillar count) | normalised pose matrices, filled in the pinned ``blob_host``, ONE host-to-device transfer per frame."""
    def __init__(self, weights_sig, src: dict, device, capacity: Optional[int], pose_host: Optional[torch.Tensor], grid: tuple):
        super().__init__(weights_sig)
        self.capacity, self.grid = capacity, grid       # rows the captured launch covers when the bucket rule sized it, else None (this frame's rows) | (ny, nx, voxel size)
        self.pose_key = _pose_key(src)                  # (aligned frames never come with host poses: the matrices are the corrector's)
        pw = src[self.pose_key]
        n_aff = pw.numel() // 16 * 6 if pose_host is not None else 0
        self.blob_host = torch.zeros(4 + n_aff, dtype=torch.int64).pin_memory()
        self.blob = torch.zeros(4 + n_aff, dtype=torch.int64, device=device)
        self.record = ops.PillarFrameRecord(self.blob[:4], self.blob_host[:4], capacity if capacity is not None else int(src["voxel_features"].shape[0]))
        self.proto: Optional[dict] = {name: src[name] for name in _PILLAR_ARRAYS}      # the capture-time arrays (shapes / dtypes only)
        if pose_host is not None:
            shape = tuple(pw.shape[:-2]) + (2, 3)
            self.affine_view = self.blob[4:].view(torch.float64).view(shape)      # [B, L, L, 2, 3]: host-normalised poses as the device sees them
            self.affine_host = self.blob_host[4:].view(torch.float64).numpy().reshape(shape)
        else:
            self.inputs[self.pose_key] = torch.zeros_like(pw, device=device)

    def stage(self, src: dict, pose_host: Optional[torch.Tensor]) -> None:
        """(The lane's previous frame has been collected: the pinned words are free.)  Host poses are normalised here (transformation_utils.py:69-91, the device's bits)."""
        self.record.set(src["voxel_features"], src["voxel_num_points"], src["voxel_coords"])
        if self.affine_view is not None:
            assert pose_host is not None, "a slot captured with host poses serves frames that carry them (FramePipeline._slot_key)"
            normalize_pairwise_np(pose_host.numpy(), *self.grid, out=self.affine_host)
        else:
            self.inputs[self.pose_key].copy_(src[self.pose_key], non_blocking=True)
        self.blob.copy_(self.blob_host, non_blocking=True)

    def batch(self, record: List[int]) -> dict:
        b = {"processed_lidar": dict(self.proto, pillar_frame=self.record), "record_len": record, self.pose_key: self.inputs.get(self.pose_key)}
        if self.affine_view is not None:
            b["normalized_affine_matrix"] = self.affine_view
        return b


class FramePipeline:
    """``submit(batch)`` enqueues one frame (``batch`` = what the reference passes to ``model(...)``: ``batch_data['ego']``),
    returns the frames that completed; ``drain()`` returns the rest.  ``run(frames)`` = the whole loop, results in order.

    ``exchange``: optional per-lane callables ``feats -> (feats, rows)`` (``FrameRing.exchange``) placed between the per-agent encoder and the ego tail (the
    agent-sharded multi-GPU schedules of ``coalign_amd.sharded`` plug in here).  With ``graph`` a lane then replays TWO graphs per frame -- the encoder
    and the ego tail -- with the collective enqueued between them (round 5: ~150 eager launches per frame were 1.35 ms of host time beside a 1.9 ms frame);
    the exchange must return the same buffers on every call (FrameRing / AgentGather without a wire dtype do).

    ``aligner`` (``box_align.Aligner``): frames carry ``lidar_poses`` [N, 6] and are pose-corrected inside the frame (module docstring); ``pairwise_t_matrix`` is
    ignored and may be absent.  One sample per frame (a corrector is one sample), at most ``min(8, max_cav)`` agents, the stage-1 anchors on the fusion model's
    canvas (the eager driver's ``processed_lidar_stage1`` form is not offered), no ``exchange`` (multi-rank frames would need every agent's boxes on the ego rank):
    each is a ``ValueError``.  Every captured slot, and every lane in eager mode, owns a ``PoseCorrector``; the stage-1 encoder gets a per-slot canvas like the
    fusion model's.  ``PointPillarUncertainty`` does not take frame records (its encoder is on the dense-canvas route): the first capture then switches the pipeline
    to copied frames, which ``frames_copied`` shows.  In eager mode an aligned lane's previous frame is collected before the lane is reused (its corrector's
    outputs are the lane's).  ``submit_points`` works with an aligner: the voxeliser's pillars feed both encoders."""

    def __init__(self, model, post_processor: VoxelPostprocessor, anchor_box, *, lanes: int = 4, result_lag: int = 1,
                 graph: bool = False, device=None, transformation_matrix: Optional[torch.Tensor] = None,
                 exchange: Optional[Sequence[Callable]] = None, preprocessor=None, points_per_cloud: int = 131072,
                 ego_filter: bool = True, filter_range: Optional[Sequence[float]] = None, pillar_buckets: bool = True,
                 streams: Optional[Sequence[torch.cuda.Stream]] = None, queue_depth: int = 1, aligner=None):
        self.model = model
        self.aligner = aligner
        if aligner is not None:
            self._check_aligner(model, post_processor, aligner, exchange)
        self.pillar_buckets = bool(pillar_buckets)               # ragged from-pillars frames share a capacity-sized graph (_slot_key)
        self._sig_tensors: Optional[list] = None                 # cached parameter / buffer list of _weights_signature
        self._sig_age = 0
        self._sd_hook = self._sd_hook1 = None                    # removed again in close(): a hook on a model must not keep every pipeline built on it alive
        if hasattr(model, "register_load_state_dict_post_hook"):
            me = weakref.ref(self)

            def _on_load(*_):
                p = me()
                if p is not None:
                    p._sig_tensors = None
            self._sd_hook = model.register_load_state_dict_post_hook(_on_load)
        stage1 = getattr(aligner, "stage1_model", None)
        if hasattr(stage1, "register_load_state_dict_post_hook"):      # (set up on its own: the fusion model need not be a module for the stage-1 model to be one)
            me1 = weakref.ref(self)

            def _on_load1(*_):
                p = me1()
                if p is not None:
                    p._sig_tensors = None
            self._sd_hook1 = stage1.register_load_state_dict_post_hook(_on_load1)
        self.pp = post_processor
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        if self.device.type != "cuda":
            raise ops.hip.CoalignHipError("FramePipeline runs on the MI355X only (the hot path has no CPU implementation)")
        # ``queue_depth`` (round 5): frames QUEUED per HIP stream.  ``lanes`` streams x ``queue_depth`` pipeline lanes: lane i runs on stream i mod lanes with graphs and
        # result buffers of its own, so a stream's next frames are enqueued while its current one still runs -- the stream never waits for the host between frames
        # (collect, stage, launch: 0.15-0.2 ms per frame otherwise).  With ``result_lag = lanes * queue_depth - 1`` the host only ever waits for the oldest frame.
        self.n_streams = max(1, int(lanes))
        self.queue_depth = max(1, int(queue_depth))
        self.n_lanes = self.n_streams * self.queue_depth
        self.graph = bool(graph)
        if exchange is not None and len(exchange) != self.n_lanes:
            raise ValueError("one exchange callable per lane")
        self.exchange = exchange
        # a lane's decode buffers / pinned result words are rewritten by its next replay: collect before that
        self.result_lag = max(0, min(int(result_lag), self.n_lanes - 1)) if self.graph else max(0, int(result_lag))
        a = anchor_box if torch.is_tensor(anchor_box) else torch.from_numpy(np.asarray(anchor_box))
        T = torch.eye(4) if transformation_matrix is None else torch.as_tensor(transformation_matrix)
        self.meta = {"ego": {"transformation_matrix": T.to(device=self.device, dtype=torch.float32), "anchor_box": a}}
        # One HIP stream per lane.  ``streams``: lane streams to REUSE (>= lanes of them) -- a process that builds several pipelines one after the other
        # (the bench's sections, a service swapping models) should hand the same streams to each: the runtime maps streams onto a small number of
        # hardware queues (four by default), and lanes of a new pipeline that land on a queue an older pipeline's idle stream still owns, or on each
        # other's, serialise (measured: the same from-points loop 441 vs 493 frames/s depending on how many streams earlier sections had left behind).
        if streams is not None:
            if len(streams) < self.n_streams:
                raise ValueError(f"{self.n_streams} lane streams needed, got {len(streams)}")
            base = list(streams[: self.n_streams])
        else:
            with torch.cuda.device(self.device):
                base = [torch.cuda.Stream(device=self.device) for _ in range(self.n_streams)]
        self.streams = [base[i % self.n_streams] for i in range(self.n_lanes)]
        with torch.cuda.device(self.device):
            ops.sp_range_flag(self.device)                        # the SplitMap range word exists before any graph is captured (its pointer is baked into the capture)
        # (only now, with every argument validated, is the model touched)
        self._vfe_flag = None
        if hasattr(model, "pillar_vfe"):
            self._vfe_flag = model.pillar_vfe.persistent_canvas
            model.pillar_vfe.persistent_canvas = True        # every lane runs its backbone before it encodes its next frame (close() restores)
        self._vfe1_flag = None
        if aligner is not None and hasattr(aligner.stage1_model, "pillar_vfe"):      # the stage-1 encoder: the same treatment
            self._vfe1_flag = aligner.stage1_model.pillar_vfe.persistent_canvas
            aligner.stage1_model.pillar_vfe.persistent_canvas = True
        self._lane_correctors: List[Optional[object]] = [None] * self.n_lanes      # eager mode: (PoseCorrector, pinned block) per lane
        self.alignments: "collections.deque" = collections.deque(maxlen=65536)     # per collected aligned frame: (index, status word, corrected lidar_poses [N, 6] ndarray)
        self.pp.buffer_sets = max(int(getattr(self.pp, "buffer_sets", 2)), self.result_lag + 2)
        self._slots: List[Dict[tuple, _GraphSlot]] = [dict() for _ in range(self.n_lanes)]
        self.max_graphs_per_lane = 4                              # distinct input shapes kept captured per lane (oldest evicted)
        self._bucket_seen: List[Dict[tuple, tuple]] = [dict() for _ in range(self.n_lanes)]      # per lane: capacity bucket -> the first key seen in it (_slot_key)
        # frames read in place through a device record (no input copies); switched off for good when the model's route turns out not to take one
        # (an explicit capability of the model class -- ADVICE r05: a model whose forward builds its own batch_dict would drop the record and the captured graph would keep
        #  reading the FIRST frame's arrays; PillarVFE raises FrameRecordUnsupported when a record reaches a route that cannot take it, which switches this off as well)
        self._records_ok = FRAME_RECORDS and bool(getattr(model, "accepts_pillar_frame", False)) and hasattr(model, "pillar_vfe") and hasattr(model, "scatter")
        self.frames_in_place = self.frames_copied = 0             # graph-mode frames read through a device record / copied into the graph's input buffers
        self._host_poses = self._records_ok and bool(getattr(model, "accepts_normalized_affine", False)) and hasattr(model, "voxel_size")
        self._grid = (model.scatter.ny, model.scatter.nx, float(model.voxel_size[0])) if self._host_poses else None      # what the host normalisation of poses needs, read HERE: a model that declares accepts_normalized_affine has scatter.ny / .nx and voxel_size
        self.graphs_captured = 0
        self._lane_busy: List[Optional[int]] = [None] * self.n_lanes          # frame index whose result still sits in the lane's buffers
        self._pending: "collections.deque" = collections.deque()              # (index, handle, keep-alive batch, submit time)
        self._count = 0
        self.host_enqueue_s = 0.0
        self.latencies_ms: "collections.deque" = collections.deque(maxlen=65536)      # per collected frame: submit -> detections on the host (bounded: a long-running service)
        # ---- submit_points: the voxeliser in front of the model
        self.preprocessor = preprocessor                          # coalign_amd.preprocess.SpVoxelPreprocessor (grid + voxel limits)
        self.points_per_cloud = int(points_per_cloud)             # slot size of one cloud in the staging buffer (NaN padded)
        self._voxelizer = (preprocessor, bool(ego_filter), filter_range)      # _points_batch's settings
        self._staging: List[Dict[int, torch.Tensor]] = [dict() for _ in range(self.n_lanes)]      # per lane: n_clouds -> pinned [n_clouds * slot, 4]
        self._staged: List[Optional[torch.cuda.Event]] = [None] * self.n_lanes

    # ------------------------------------------------------------------------------------------------ one frame
    def _eager(self, k: int, batch: dict, record: List[int]) -> PostProcessHandle:
        if batch.get("_point_offsets") is not None:
            with ops.timed("stage_h2d+voxelize"):
                pts = batch["_points_pinned"].to(self.device, non_blocking=True)
                self._staged[k] = self.streams[k].record_event()
                key = "lidar_poses" if self.aligner is not None else "pairwise_t_matrix"
                batch = _points_batch(self._voxelizer, pts, batch["_point_offsets"], record, batch[key].to(self.device, non_blocking=True), key)
        if self.aligner is not None:
            if self._lane_correctors[k] is None:
                self._lane_correctors[k] = self._new_corrector()
            with ops.timed("stage_pose_correction"):
                batch = self._aligned(self._lane_correctors[k], batch, record)
        with ops.timed("stage_encode(pillars+backbone)"):
            feats, affine = self.model.encode(batch)
        rows = None
        if self.exchange is not None:
            with ops.timed("stage_exchange"):
                feats, rows = self.exchange[k](feats)
        with ops.timed("stage_fuse_and_heads"):
            # (an exchange that gathers agents encoded elsewhere says how many the ego tail sees: AgentGather, bench.py --mode gather)
            out = self.model.fuse_and_head(feats, host_ints(batch["tail_record_len"]) if "tail_record_len" in batch else record, affine, rows)
        with ops.timed("stage_post_process(enqueue)"):
            return self.pp.post_process_async(self.meta, {"ego": out}, side_stream=True)

    # ------------------------------------------------------------------------------------------------ aligned frames
    @staticmethod
    def _check_aligner(model, post_processor, aligner, exchange) -> None:
        if exchange is not None:
            raise ValueError("FramePipeline(aligner=...) with an exchange: multi-rank frames would need every agent's stage-1 boxes on the ego rank")
        if not 1 <= aligner.max_cav:
            raise ValueError("aligner.max_cav must be at least 1")
        aa = aligner.post_processor.params["anchor_args"]
        vfe = getattr(model, "pillar_vfe", None)
        if vfe is not None:
            rng, grid = [float(v) for v in vfe.point_cloud_range], (vfe.ny, vfe.nx)
        else:
            fa = post_processor.params["anchor_args"]
            rng, grid = [float(v) for v in fa["cav_lidar_range"]], (int(fa["H"]), int(fa["W"]))
        if [float(v) for v in aa["cav_lidar_range"]] != rng or (int(aa["H"]), int(aa["W"])) != grid:
            raise ValueError(f"the stage-1 anchors cover range {list(aa['cav_lidar_range'])} / grid {(aa['H'], aa['W'])}, the fusion model's canvas {rng} / {grid}: "
                             "the pipeline feeds both encoders the same pillars (inference_intermediate_fusion_aligned takes processed_lidar_stage1)")

    def _new_corrector(self) -> tuple:
        """-> (PoseCorrector, pinned block) of one owner.  Block: word 0 the status (int32 in an 8-byte word), then the corrected poses, 6 float64 per agent."""
        return self.aligner.corrector(self.device), torch.zeros(1 + 6 * ops.ALIGN_MAX_AGENTS, dtype=torch.int64).pin_memory()

    def _aligned(self, owner: tuple, batch: dict, record: List[int]) -> dict:
        """The chain on the batch's pillars and noisy poses -> the batch the fusion model runs on (the corrector's matrices in place of the frame's); the status
        word and the corrected poses follow to the owner's pinned block behind the three launches (read when the frame is collected)."""
        from .box_align import correct_frame_poses
        corrector, host = owner
        al = self.aligner
        fixed = correct_frame_poses(al.stage1_model, al.post_processor, al.anchor_box, corrector, batch["processed_lidar"], batch["lidar_poses"], record_len=record)
        host[:1].view(torch.int32)[:1].copy_(fixed["status"], non_blocking=True)
        poses = fixed["lidar_poses"]                                # [N, 6]: the frame's agents
        host[1: 1 + poses.numel()].view(torch.float64).copy_(poses.reshape(-1), non_blocking=True)
        return dict(batch, pairwise_t_matrix=fixed["pairwise_t_matrix"], normalized_affine_matrix=fixed["normalized_affine_matrix"])

    def _slot_batch(self, slot: _GraphSlot, record: List[int]) -> dict:
        """What the fusion model is captured on: the slot's batch -- through the slot's corrector when frames are aligned (the one seam of the feature)."""
        batch = slot.batch(record)
        if self.aligner is None:
            return batch
        if slot.corrector is None:
            slot.corrector, slot.align_host = self._new_corrector()
        return self._aligned((slot.corrector, slot.align_host), batch, record)

    def _with_slot_canvas(self, slot: _GraphSlot, fn):
        """Run ``fn()`` with the encoder's canvas bookkeeping pointed at the slot's own: a graph bakes its launches, the persistent canvas's "rows of the
        previous frame" bookkeeping included, so every captured frame gets a canvas / cell map / slot list of its own, touched by nothing but its own
        replays (warm-up call first: the capture then bakes "clear M rows, encode M pillars", which is what every replay needs)."""
        pairs = [(getattr(self.model, "pillar_vfe", None), slot.canvas_cache)]
        if self.aligner is not None:
            pairs.append((getattr(self.aligner.stage1_model, "pillar_vfe", None), slot.canvas_cache1))
        pairs = [(vfe, cache) for vfe, cache in pairs if vfe is not None]
        keep = [(vfe.persistent_canvas, vfe.__dict__.get("_canvas_cache")) for vfe, _ in pairs]
        try:
            for vfe, cache in pairs:
                vfe.persistent_canvas, vfe.__dict__["_canvas_cache"] = True, cache
            return fn()
        finally:
            for (vfe, _), (flag, cache) in zip(pairs, keep):
                vfe.persistent_canvas = flag
                if cache is None:
                    vfe.__dict__.pop("_canvas_cache", None)
                else:
                    vfe.__dict__["_canvas_cache"] = cache

    def _post_process(self, slot: _GraphSlot, out: dict) -> None:
        if slot.buf is None:
            slot.buf = self.pp.decode_buffers({"ego": out})
        self.pp.enqueue(self.meta, {"ego": out}, slot.buf)

    def _frame_body(self, slot: _GraphSlot, record: List[int]) -> None:
        self._post_process(slot, self._with_slot_canvas(slot, lambda: self.model(self._slot_batch(slot, record))))

    def _encode_body(self, slot: _GraphSlot, record: List[int]) -> None:
        slot.feats, slot.affine = self._with_slot_canvas(slot, lambda: self.model.encode(slot.batch(record)))
        slot.feats = list(slot.feats)

    def _tail_body(self, slot: _GraphSlot, feats, rows) -> None:
        self._post_process(slot, self.model.fuse_and_head(list(feats), slot.tail_record, slot.affine, rows))

    @staticmethod
    def _quiesce_collectives(stream) -> None:
        """Before a capture on a stream a collective has just run on: wait for the stream AND for the collective backend's watchdog to retire the finished work.
        RCCL's process group records a collective's end event on the caller's stream and its watchdog thread polls that event every 100 ms until it has seen it
        complete; ROCm's hipEventQuery refuses an event whose stream is capturing at that moment (hipErrorCapturedEvent), which ends the watchdog -- and with it the
        process -- even under the thread-local capture mode (round 6: 1 run in 12 of tests/test_round6_gpu.py::test_rccl_world_of_one_*, whenever a poll fell into
        the ~20 ms of a capture).  Three poll periods after the stream has drained no finished work is left to poll.  Captures happen once per (lane, shape)."""
        stream.synchronize()
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
                time.sleep(0.35)
        except Exception:      # noqa: BLE001  (no process group: nothing polls)
            pass

    def _capture(self, k: int, slot: _GraphSlot, record: List[int], tail_rec: Optional[tuple]) -> None:
        """Eager warm-up on the lane (MIOpen find, weight folds, anchors, canvases, buffers, the exchange's receive buffers), then the capture: the whole frame as ONE graph,
        or, with an ``exchange``, encoder graph | collective (eager, on the lane's stream) | tail graph in thread-local error mode (the collective's watchdog polls events)."""
        stream = self.streams[k]
        if self.exchange is None:
            self._frame_body(slot, record)
            stream.synchronize()
            slot.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(slot.graph, stream=stream):
                self._frame_body(slot, record)
            return
        slot.tail_record = list(record if tail_rec is None else tail_rec)
        self._encode_body(slot, record)
        feats, rows = self.exchange[k](slot.feats)
        self._tail_body(slot, feats, rows)
        self._quiesce_collectives(stream)
        slot.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(slot.graph, stream=stream, capture_error_mode="thread_local"):
            self._encode_body(slot, record)
        feats, rows = self.exchange[k](slot.feats)              # on the capture's output maps: these are the send buffers of every replay
        slot.recv_ptrs, slot.rows, slot.recv_keep = tuple(f.data_ptr() for f in feats), None if rows is None else list(rows), feats
        self._quiesce_collectives(stream)
        slot.tail = torch.cuda.CUDAGraph()
        with torch.cuda.graph(slot.tail, stream=stream, capture_error_mode="thread_local"):
            self._tail_body(slot, feats, rows)

    def _slot_key(self, k: int, record: List[int], tail_rec: Optional[tuple], offsets, direct: bool, pose_host: bool, src: dict) -> Tuple[tuple, Optional[int]]:
        """-> (key of the captured frame that serves this input on lane ``k``, rows of its pillar buffers or None = this frame's own).  Ragged from-pillars frames:
        the first shape of a capacity bucket (next power of two, >= 4096 rows) is captured exactly (a stream of equal shapes -- the bench pool -- keeps the graph that
        bakes its count); the SECOND different shape captures ONE graph with capacity-sized inputs and the count on the device (PillarVFE's voxel_count_dev form, cells
        not assumed unique), which serves every other count of that bucket: <= 2 graphs per lane.  ``pillar_buckets=False``: every shape is captured exactly."""
        pk = _pose_key(src)                                      # (an aligned frame and a plain one never share a captured graph)
        key = (tuple(record), tail_rec, None if offsets is None else tuple(offsets), direct, pose_host, pk) + tuple((tuple(t.shape), str(t.dtype)) for t in src.values())
        if offsets is not None or not self.pillar_buckets or key in self._slots[k]:
            return key, None
        cap = max(4096, 1 << max(int(src["voxel_features"].shape[0]) - 1, 0).bit_length())
        bkey = (tuple(record), tail_rec, "bucket", cap, direct, pose_host, tuple(src["voxel_features"].shape[1:]), pk, tuple(src[pk].shape))
        if self._bucket_seen[k].setdefault(bkey, key) != key or bkey in self._slots[k]:      # a second shape of this bucket: the capacity-sized graph from here on
            return bkey, cap
        return key, None                                         # first shape of its bucket: exact capture

    def _frame_source(self, batch: dict, offsets) -> Tuple[dict, bool, Optional[torch.Tensor], Callable]:
        """-> (the frame's inputs, whether the pillar launch reads them in place (a record), host poses to normalise or None, its form's ``(weights_sig, capacity) -> slot``)."""
        pk = "lidar_poses" if self.aligner is not None else "pairwise_t_matrix"
        if offsets is not None:
            src = {"points": batch["_points_pinned"], pk: batch[pk]}
            return src, False, None, lambda sig, cap: _PointsSlot(sig, src, self.device, offsets, self._voxelizer)
        src = dict({name: batch["processed_lidar"][name] for name in _PILLAR_ARRAYS}, **{pk: batch[pk]})
        direct = self._records_ok and ops.PillarFrameRecord.admits(src["voxel_features"], src["voxel_num_points"], src["voxel_coords"], self.device)
        pose_host = batch.get("pairwise_t_matrix_host") if direct and self._host_poses and self.aligner is None else None
        # (the host copy stands in for the device matrix only when both are the dataset's float64 matrices of one shape: a float32 device matrix normalises to other bits)
        if pose_host is not None and (pose_host.is_cuda or pose_host.dtype != torch.float64 or src["pairwise_t_matrix"].dtype != torch.float64
                                      or tuple(pose_host.shape) != tuple(src["pairwise_t_matrix"].shape)):
            pose_host = None
        if direct:
            return src, True, pose_host, lambda sig, cap: _PillarRecordSlot(sig, src, self.device, cap, pose_host, self._grid)
        return src, False, None, lambda sig, cap: _PillarCopySlot(sig, src, self.device, cap)

    def _graphed(self, k: int, batch: dict, record: List[int]) -> PostProcessHandle:
        offsets = batch.get("_point_offsets")
        src, direct, pose_host, new_slot = self._frame_source(batch, offsets)
        # (multi-rank frames: the tail graph bakes the agent grouping the ego sees -- another rank dropping an agent changes it while this rank's record stays the same)
        tail_rec = tuple(host_ints(batch["tail_record_len"])) if (self.exchange is not None and "tail_record_len" in batch) else None
        key, cap = self._slot_key(k, record, tail_rec, offsets, direct, pose_host is not None, src)
        # a graph holds raw pointers to the folded / packed weight images of its capture: re-capture when any parameter or buffer has been replaced or written since
        sig = self._weights_signature()
        if key in self._slots[k] and self._slots[k][key].weights_sig != sig:
            del self._slots[k][key]
        slot = self._slots[k].get(key)
        if slot is None:
            if len(self._slots[k]) >= self.max_graphs_per_lane:      # bound the memory captured frames hold (one private pool + canvas each): the oldest leaves
                del self._slots[k][next(iter(self._slots[k]))]
            slot = new_slot(sig, cap)
            slot.stage(src, pose_host)
            try:
                self._capture(k, slot, record, tail_rec)
            except ops.FrameRecordUnsupported:
                # (raised by the eager warm-up, before any capture has begun: this model's encoder reads its arrays directly -- copy frames in from now on)
                self._records_ok = self._host_poses = False
                return self._graphed(k, batch, record)
            if direct:
                slot.proto = None                               # (the capture-time arrays gave shapes and dtypes only: not kept alive for the slot's lifetime)
            self.graphs_captured += 1
            self._slots[k][key] = slot                          # only a slot whose capture succeeded is ever looked up again
        self.frames_in_place += slot.record is not None
        self.frames_copied += slot.record is None
        slot.stage(src, pose_host)
        if offsets is not None:
            self._staged[k] = self.streams[k].record_event()        # the pinned staging buffer may be refilled once this has passed
        return self._replay(k, slot)

    def _replay(self, k: int, slot: _GraphSlot) -> PostProcessHandle:
        slot.replays += 1
        if slot.replays >= ops.SPARSE_TAG_RESET_AFTER:          # the 32-bit frame tag of the slot's sparse canvas must not wrap: re-zero the stamp map between replays
            with torch.cuda.stream(self.streams[k]):
                ops.reset_sparse_canvases(slot.canvas_cache)
                ops.reset_sparse_canvases(slot.canvas_cache1)
            slot.replays = 0
        slot.graph.replay()
        if slot.tail is not None:                               # multi-rank frame: the collective between the encoder's and the tail's replay
            feats, rows = self.exchange[k](slot.feats)
            if tuple(f.data_ptr() for f in feats) != slot.recv_ptrs or (None if rows is None else list(rows)) != slot.rows:
                raise ops.hip.CoalignHipError("the exchange returned other buffers / another row table than the tail graph was captured on "
                                              "(a wire dtype or a changing schedule): run this pipeline with graph=False")
            slot.tail.replay()
        handle = PostProcessHandle(self.pp, slot.buf, self.streams[k].record_event())
        handle.align_host = slot.align_host
        return handle

    def _weights_signature(self) -> tuple:
        # The tensor list is cached (walking the module tree on every frame cost ~50 us of host time): it is rebuilt after a load_state_dict (hook),
        # and every 16 frames anyway (round 6, VERDICT r05: 256 before; ~3 us per frame amortised) -- parameters replaced as OBJECTS by module surgery change the
        # list itself and are noticed within 16 frames; in-place writes and storage swaps of the cached tensors show in (data_ptr, _version) at once.
        self._sig_age += 1
        if self._sig_tensors is None or self._sig_age >= 16:
            self._sig_tensors = list(self.model.parameters()) + list(self.model.buffers())
            stage1 = getattr(self.aligner, "stage1_model", None)
            if hasattr(stage1, "parameters"):                  # a captured aligned frame bakes the stage-1 model's weight images too
                self._sig_tensors += list(stage1.parameters()) + list(stage1.buffers())
            self._sig_age = 0
        return tuple((id(t), t.data_ptr(), t._version) for t in self._sig_tensors)

    def _aligned_frame(self, batch: dict) -> dict:
        """Checks of a frame submitted to an aligned pipeline -> the batch with ``lidar_poses`` as a float64 [N, 6] tensor (host or device) and without the
        pose matrices the corrector replaces."""
        record = host_ints(batch["record_len"])
        if len(record) != 1:
            raise ValueError(f"an aligned frame is one sample (a corrector is one sample): record_len = {record}")
        limit = min(ops.ALIGN_MAX_AGENTS, self.aligner.max_cav)
        if not 1 <= record[0] <= limit:
            raise ValueError(f"{record[0]} agents: an aligned frame has 1 .. min({ops.ALIGN_MAX_AGENTS}, max_cav = {self.aligner.max_cav}) agents")
        if batch.get("lidar_poses") is None:
            raise ValueError("a frame submitted to FramePipeline(aligner=...) carries 'lidar_poses' [N, 6]")
        poses = batch["lidar_poses"]
        poses = (poses if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses))).to(torch.float64).contiguous()
        if tuple(poses.shape) != (record[0], 6):
            raise ValueError(f"lidar_poses {tuple(poses.shape)}: expected ({record[0]}, 6) = x, y, z, roll, yaw, pitch (degrees) per agent")
        batch = {k: v for k, v in batch.items() if k not in ("pairwise_t_matrix", "pairwise_t_matrix_host", "normalized_affine_matrix")}
        return dict(batch, record_len=record, lidar_poses=poses)

    # ------------------------------------------------------------------------------------------------ the loop
    def submit_points(self, frame: dict) -> List[FrameResult]:
        """One frame from raw clouds in HOST memory: ``frame`` = {"clouds": [ndarray / CPU tensor [n_i, 4] float32 per cav, ego first],
        "record_len": [N] (or [n_1, n_2, ...] for a batch), "pairwise_t_matrix": float64 [B, L, L, 4, 4]} (with an ``aligner``: "lidar_poses" [N, 6] instead).  The clouds are packed into the
        lane's pinned staging buffer (``points_per_cloud`` slots per cloud, the tail NaN: the voxeliser rejects NaN coordinates) and the
        frame goes: async copy -> voxelise -> encode -> fuse -> heads -> decode -> NMS.  Returns the frames that completed, like ``submit``."""
        if self.preprocessor is None:
            raise ValueError("submit_points needs FramePipeline(preprocessor=SpVoxelPreprocessor(...)): grid, max points / voxels")
        if self.exchange is not None:
            raise ValueError("submit_points is the single-GPU feeder path")
        t_sub = time.perf_counter()
        clouds = frame["clouds"]
        n, S = len(clouds), self.points_per_cloud
        k = self._count % self.n_lanes
        done: List[FrameResult] = []
        if self.graph and self._lane_busy[k] is not None:
            done += self._collect_through(self._lane_busy[k])
        stage = self._staging[k].get(n)
        if stage is None:
            stage = self._staging[k][n] = torch.empty((n * S, 4), dtype=torch.float32).pin_memory()
        if self._staged[k] is not None:
            self._staged[k].synchronize()                        # the previous copy out of this buffer has left the host
        view = stage.view(n, S, 4).numpy()
        for i, c in enumerate(clouds):
            c = c.numpy() if torch.is_tensor(c) else np.asarray(c, dtype=np.float32)
            if c.shape[0] > S:
                raise ValueError(f"cloud {i} has {c.shape[0]} points; FramePipeline(points_per_cloud={S}) is the slot size")
            view[i, : c.shape[0]] = c
            view[i, c.shape[0]:] = np.nan
        pk = "lidar_poses" if self.aligner is not None else "pairwise_t_matrix"
        pw = frame[pk]
        pw = pw if torch.is_tensor(pw) else torch.from_numpy(np.asarray(pw))
        batch = {"record_len": frame["record_len"], pk: pw, "_points_pinned": stage, "_point_offsets": [i * S for i in range(n + 1)]}
        return done + self.submit(batch, _t_submit=t_sub)

    def submit(self, batch: dict, _t_submit: Optional[float] = None) -> List[FrameResult]:
        """Enqueue one frame; -> the frames that completed.  LIFETIME OF THE INPUTS: in graph mode a float32 / int32 contiguous frame on the lane's device is read
        IN PLACE by the pillar launch (no input copy), so ``batch['processed_lidar']`` must stay UNMODIFIED until this frame's result has come back -- up to
        ``result_lag`` submits later (the pipeline keeps the tensors referenced; it cannot keep a caller from refilling a preallocated batch).  A caller that
        reuses its input buffers passes ``COALIGN_FRAME_RECORDS=0`` (every frame is copied into the graph's own buffers, as in rounds 2-4) or waits for the result."""
        t0 = time.perf_counter()
        t_sub = t0 if _t_submit is None else _t_submit
        if self.aligner is not None:
            batch = self._aligned_frame(batch)
        idx = self._count
        k = idx % self.n_lanes
        self._count += 1
        done: List[FrameResult] = []
        if (self.graph or self.aligner is not None) and self._lane_busy[k] is not None:      # (an aligned lane's corrector outputs and pinned block are the lane's, eager mode included)
            done += self._collect_through(self._lane_busy[k])
            t0 = time.perf_counter()
        record = host_ints(batch["record_len"])
        batch = dict(batch, record_len=record)
        stream = self.streams[k]
        with torch.cuda.device(self.device), torch.no_grad():
            stream.wait_stream(torch.cuda.current_stream(self.device))      # inputs were produced on the caller's stream
            with torch.cuda.stream(stream):
                handle = self._graphed(k, batch, record) if self.graph else self._eager(k, batch, record)
        self._lane_busy[k] = idx
        if self.aligner is not None:                            # where this frame's status word and corrected poses land, and how many poses
            owner = self._lane_correctors[k] if not self.graph else None
            handle.align = (owner[1] if owner is not None else handle.align_host, sum(record))
        self._pending.append((idx, handle, batch, t_sub))       # the batch stays referenced until its frame has completed
        self.host_enqueue_s += time.perf_counter() - t0         # launch work only: waiting for older frames' results is GPU time
        while len(self._pending) > self.result_lag:
            done.append(self._pop())
        return done

    def _pop(self) -> FrameResult:
        idx, handle, _keep, t_sub = self._pending.popleft()
        boxes, scores = handle.result()
        align = getattr(handle, "align", None)
        if align is not None:
            host, n = align
            self.alignments.append((idx, int(host[:1].view(torch.int32)[0]), host[1: 1 + 6 * n].view(torch.float64).numpy().reshape(n, 6).copy()))
        self.latencies_ms.append((time.perf_counter() - t_sub) * 1e3)
        k = idx % self.n_lanes
        if self._lane_busy[k] == idx:
            self._lane_busy[k] = None
        return idx, boxes, scores

    def _collect_through(self, idx: int) -> List[FrameResult]:
        out = []
        while self._pending and self._pending[0][0] <= idx:
            out.append(self._pop())
        return out

    def drain(self) -> List[FrameResult]:
        return self._collect_through(self._count)

    def run(self, frames: Iterable[dict]) -> List[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]]:
        """The reference's loop body for every frame of ``frames``; -> [(pred_box3d, scores)] in input order."""
        results: List[FrameResult] = []
        for batch in frames:
            results += self.submit(batch)
        results += self.drain()
        assert [r[0] for r in results] == sorted(r[0] for r in results)
        return [(b, s) for _, b, s in results]

    def synchronize(self) -> None:
        for s in self.streams:
            s.synchronize()

    def range_exceeded(self, clear: bool = True) -> bool:
        """True if, since the last clearing call, a 3x3 layer wrote a value beyond the fp16 split's operating range (|x| > 65504) into a SplitMap: the
        default arithmetic clamps there instead of overflowing, and a model that does so wants ``COALIGN_CONV_EMU=3``.  Synchronises."""
        self.synchronize()
        return ops.sp_range_exceeded(self.device, clear=clear)

    def close(self) -> None:
        """Collect what is pending, drop the captured graphs (and the canvases they own) and give the model's ``persistent_canvas`` flag back."""
        self.drain()
        self.synchronize()
        for d in self._slots:
            d.clear()
        if self._sd_hook is not None:
            self._sd_hook.remove()
            self._sd_hook = None
        if self._vfe_flag is not None and hasattr(self.model, "pillar_vfe"):
            self.model.pillar_vfe.persistent_canvas = self._vfe_flag
            self.model.pillar_vfe.__dict__.pop("_canvas_cache", None)
        if self._sd_hook1 is not None:
            self._sd_hook1.remove()
            self._sd_hook1 = None
        if self._vfe1_flag is not None:
            self.aligner.stage1_model.pillar_vfe.persistent_canvas = self._vfe1_flag
            self.aligner.stage1_model.pillar_vfe.__dict__.pop("_canvas_cache", None)
        self._lane_correctors = [None] * self.n_lanes
