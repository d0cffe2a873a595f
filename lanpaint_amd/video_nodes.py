"""LanPaint_VideoMaskEditor: the reference's video mask editor node (nodes.py:890-995) with its masks built on the GPU.

Same protocol as the reference -- inputs, widgets, return types -- so workflows saved with the reference's editor (its
web/ frontend writes the `keyframes` and `audio_mask` widgets) run unchanged.  The keyframe PNGs are read on the host, the
per-frame masks are made on the HIP device by lanpaint_amd.videomask.interpolate_masks; the MASK outputs are host tensors,
as ComfyUI and the reference hand them on.

This module has its own NODE_CLASS_MAPPINGS: merge them with lanpaint_amd.nodes' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import os

import torch

from . import videomask

VIDEO_EXTENSIONS = (".mp4", ".webm", ".mov", ".mkv", ".avi", ".m4v", ".gif")


def _video_from_file():
    try:
        from comfy_api.latest._input_impl.video_types import VideoFromFile
    except Exception:
        return None
    return VideoFromFile


def _input_videos():
    try:
        import folder_paths
        root = folder_paths.get_input_directory()
        return sorted(f for f in os.listdir(root)
                      if os.path.isfile(os.path.join(root, f)) and f.lower().endswith(VIDEO_EXTENSIONS))
    except Exception:
        return []


class LanPaint_VideoMaskEditor:
    """Loads a video like LoadVideo (the VIDEO output is the file, not decoded) and outputs the per-frame video mask
    [F, H, W] and audio mask [F] painted in the mask editor (1 = regenerate, 0 = keep)."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "video": (_input_videos(), {"video_upload": True,
                                        "tooltip": "Source video file; returned as the video output and shown by the mask editor."}),
            "keyframes": ("STRING", {"default": "{}", "multiline": True,
                                     "tooltip": "Hidden: keyframe mask files {\"frame\": \"file.png\"}, written by the mask editor."}),
            "audio_mask": ("STRING", {"default": "[]", "multiline": True,
                                      "tooltip": "Hidden: audio inpainting intervals [{\"start\": s, \"end\": e}] in seconds, "
                                                 "written by the mask editor."}),
        }}

    RETURN_TYPES = ("VIDEO", "MASK", "MASK")
    RETURN_NAMES = ("video", "mask", "audio_mask")
    FUNCTION = "run"
    CATEGORY = "video"
    DESCRIPTION = ("Loads a video and outputs a per-frame video inpainting mask (keyframes morphed on the GPU) and a per-frame "
                   "audio mask painted in the mask editor (1 = regenerate, 0 = keep).")

    def run(self, video=None, keyframes="{}", audio_mask="[]"):
        if not video:
            raise ValueError("select a video file in the node first")
        VideoFromFile = _video_from_file()
        if VideoFromFile is None:
            raise RuntimeError("the video output needs the ComfyUI runtime (comfy_api)")
        import folder_paths
        vf = VideoFromFile(folder_paths.get_annotated_filepath(video))
        count = int(vf.get_frame_count())
        width, height = vf.get_dimensions()

        loaded = {}
        for idx, name in videomask.parse_keyframes_widget(keyframes).items():
            try:
                path = folder_paths.get_annotated_filepath(name)
                if path and os.path.isfile(path):
                    loaded[idx] = videomask.load_keyframe_png(path)
            except Exception:
                continue                                   # a missing or unreadable keyframe file is skipped
        if loaded:
            mask = videomask.interpolate_masks(loaded, count, size=(width, height)).cpu()
        else:
            mask = torch.zeros(count, height, width, dtype=torch.float32)

        get_fps = getattr(vf, "get_fps", None)             # renamed get_frame_rate (a Fraction) in newer ComfyUI
        fps = float(get_fps() if get_fps else vf.get_frame_rate())
        return (vf, mask, videomask.audio_mask_frames(audio_mask, count, fps))


NODE_CLASS_MAPPINGS = {"LanPaint_VideoMaskEditor": LanPaint_VideoMaskEditor}
NODE_DISPLAY_NAME_MAPPINGS = {"LanPaint_VideoMaskEditor": "LanPaint Video Mask Editor"}
