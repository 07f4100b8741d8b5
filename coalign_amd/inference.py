"""Per-frame inference drivers: the reference's
``inference_late_fusion`` / ``inference_early_fusion`` / ``inference_intermediate_fusion``
(opencood/tools/inference_utils.py:17-46, 122-173) with the dataset object reduced to what they use from it --
a post-processor.  The data layer (disk readers, collate) is outside the hot path (§8f next-4); ``gt_box_tensor`` is the
caller's, or -- when the batch carries the label keys the reference's collate emits (``object_bbx_center`` / ``_mask`` /
``object_ids`` / ``transformation_matrix_clean``) -- built by ``VoxelPostprocessor.generate_gt_bbx`` like
``dataset.post_process`` does (intermediate_fusion_dataset.py:585-606).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from .box_align import correct_frame_poses
from .postprocess import VoxelPostprocessor


def _ground_truth(batch_data: dict, post_processor: VoxelPostprocessor, supplied):
    if supplied is not None:
        return supplied
    if all("object_bbx_center" in cav for cav in batch_data.values()):
        return post_processor.generate_gt_bbx(batch_data)
    return None


def inference_late_fusion(batch_data: dict, model, post_processor: VoxelPostprocessor, gt_box_tensor: Optional[torch.Tensor] = None) -> dict:
    """One model call per cav (each on its own canvas), then ONE merged post-process: every agent's boxes are projected
    to the ego frame with its ``transformation_matrix`` and a single rotated NMS runs over the union
    (voxel_postprocessor.py:275-381).  ``batch_data``: {cav_id: {processed_lidar..., transformation_matrix, anchor_box}}."""
    output_dict = OrderedDict()
    with torch.no_grad():
        for cav_id, cav_content in batch_data.items():
            output_dict[cav_id] = model(cav_content)
        pred_box_tensor, pred_score = post_processor.post_process(batch_data, output_dict)
    return {"pred_box_tensor": pred_box_tensor, "pred_score": pred_score,
            "gt_box_tensor": _ground_truth(batch_data, post_processor, gt_box_tensor)}


def inference_early_fusion(batch_data: dict, model, post_processor: VoxelPostprocessor, gt_box_tensor: Optional[torch.Tensor] = None) -> dict:
    """``batch_data['ego']`` holds the whole (already fused / to-be-fused) frame; identity projection."""
    with torch.no_grad():
        output_dict = OrderedDict(ego=model(batch_data["ego"]))
        pred_box_tensor, pred_score = post_processor.post_process(batch_data, output_dict)
    return {"pred_box_tensor": pred_box_tensor, "pred_score": pred_score,
            "gt_box_tensor": _ground_truth(batch_data, post_processor, gt_box_tensor)}


def inference_intermediate_fusion(batch_data: dict, model, post_processor: VoxelPostprocessor, gt_box_tensor=None) -> dict:
    return inference_early_fusion(batch_data, model, post_processor, gt_box_tensor)


def inference_intermediate_fusion_aligned(batch_data: dict, model, post_processor: VoxelPostprocessor, stage1_model=None, stage1_post_processor=None,
                                          corrector=None, gt_box_tensor=None) -> dict:
    """Intermediate fusion with ONLINE pose correction (the hook of intermediate_fusion_dataset.py:301-328 moved behind a live stage-1 forward, all on the
    device): the stage-1 model over the frame's agents (``processed_lidar`` with the agent as batch index; ``processed_lidar_stage1`` when the stage-1 range
    differs) -> ``post_process_stage1_device`` -> ``corrector.correct`` on ``batch_data['ego']['lidar_poses']`` -> the fusion model with
    ``normalized_affine_matrix`` (and ``pairwise_t_matrix``) replaced by the corrected ones -> the ordinary post-process.  Returns what
    ``inference_intermediate_fusion`` returns plus ``lidar_poses_corrected`` and ``align_status`` (device tensors).  With ``corrector=None`` it IS
    ``inference_intermediate_fusion`` and touches neither stage-1 object."""
    if corrector is None:
        return inference_intermediate_fusion(batch_data, model, post_processor, gt_box_tensor)
    if stage1_model is None or stage1_post_processor is None:
        raise ValueError("pose correction needs the stage-1 model and its post-processor")
    ego = batch_data["ego"]
    with torch.no_grad():
        fixed = correct_frame_poses(stage1_model, stage1_post_processor, ego.get("anchor_box_stage1", ego["anchor_box"]), corrector,
                                    ego.get("processed_lidar_stage1", ego["processed_lidar"]), ego["lidar_poses"])
        aligned = dict(batch_data, ego=dict(ego, pairwise_t_matrix=fixed["pairwise_t_matrix"], normalized_affine_matrix=fixed["normalized_affine_matrix"]))
        result = inference_intermediate_fusion(aligned, model, post_processor, gt_box_tensor)
    result["lidar_poses_corrected"] = fixed["lidar_poses"]
    result["align_status"] = fixed["status"]
    return result
