"""AV encode / decode nodes: the two ends of the MiniMax-H3 audio+video inpainting workflow (reference nodes.py:811-878,
998-1046, 1139-1227).

Same protocol as the reference -- inputs, widgets, return types -- so saved workflows load.  AVEncode builds the nested
(video, audio) latent with its per-stream masks, which KSamplerX0Inpaint detects and samples; AVDecode decodes both streams
and merges them with the source: the frames through lp_mask_blend (blend.merge_video_with_mask), the audio through
lp_audio_merge (audio.merge_audio_with_mask).  The VAEs are the caller's objects; outputs go back to the caller's device.

ComfyUI's comfy.nested_tensor and comfy_api are imported on first use; without them the nodes raise RuntimeError.
This module has its own NODE_CLASS_MAPPINGS: merge them with lanpaint_amd.nodes' (INTEGRATION.md section 2(b)).
"""
from __future__ import annotations

import torch

from . import audio as _audio
from ._hostcall import node_device
from .blend import merge_video_with_mask


def _nested_tensor():
    try:
        from comfy.nested_tensor import NestedTensor
    except Exception:
        raise RuntimeError("the nested AV latent needs the ComfyUI runtime (comfy.nested_tensor)") from None
    return NestedTensor


def _video_types():
    try:
        from comfy_api.latest._input_impl.video_types import VideoFromComponents
        from comfy_api.latest._util.video_types import VideoComponents
    except Exception:
        raise RuntimeError("the video output needs the ComfyUI runtime (comfy_api)") from None
    return VideoFromComponents, VideoComponents


def _flat_audio_mask(audio_mask):
    """[F, 1] -> [F]; other forms are handed on unchanged (the sampler's mask preparation reads them)."""
    if audio_mask.ndim == 2 and audio_mask.shape[1] == 1:
        return audio_mask[:, 0]
    return audio_mask


class LanPaint_MiniMaxAudioEncode:
    """Encodes a ComfyUI AUDIO with the MiniMax H3 audio VAE: resampled to the VAE's rate when needed, mono made stereo,
    handed over channels-last as the VAE wrapper expects."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "audio": ("AUDIO", {"tooltip": "Audio to encode; resampled to the VAE's sample rate when it differs."}),
            "vae": ("VAE", {"tooltip": "MiniMax H3 audio VAE."}),
        }}

    RETURN_TYPES = ("LATENT",)
    RETURN_NAMES = ("latent",)
    FUNCTION = "encode"
    CATEGORY = "audio"
    DESCRIPTION = ("Encodes audio with the MiniMax H3 audio VAE (channels-last, mono upmixed to stereo). The audio inpainting "
                   "mask comes from the video mask editor, attached with SetLatentNoiseMask.")

    def encode(self, audio, vae):
        wave, rate = audio["waveform"], audio["sample_rate"]
        target = getattr(vae, "audio_sample_rate", 32000)
        if rate != target:
            if _audio.torchaudio is None:
                raise RuntimeError("torchaudio is required to resample audio for the MiniMax H3 audio VAE")
            wave = _audio.torchaudio.functional.resample(wave, rate, target)
        if wave.shape[1] == 1:
            wave = wave.expand(-1, 2, -1)
        return ({"samples": vae.encode(wave.movedim(1, -1))},)


class LanPaint_MiniMaxAudioDecode:
    """Decodes a MiniMax H3 audio latent, or the audio stream of a nested AV latent, to a ComfyUI AUDIO ([B, C, L])."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "samples": ("LATENT", {"tooltip": "An audio latent, or a nested AV latent whose audio stream is decoded."}),
            "vae": ("VAE", {"tooltip": "MiniMax H3 audio VAE."}),
        }}

    RETURN_TYPES = ("AUDIO",)
    RETURN_NAMES = ("audio",)
    FUNCTION = "decode"
    CATEGORY = "audio"
    DESCRIPTION = "Decodes a MiniMax H3 audio latent to a waveform."

    def decode(self, samples, vae):
        z = samples["samples"]
        if getattr(z, "is_nested", False):
            z = z.unbind()[-1]
        rate = getattr(vae, "audio_sample_rate_output", getattr(vae, "audio_sample_rate", 32000))
        return ({"waveform": vae.decode(z).movedim(-1, 1), "sample_rate": rate},)


class LanPaint_AVEncode:
    """Encodes a video's frames and audio track into one nested AV latent carrying the video mask and the audio mask, in
    place of GetVideoComponents -> VAEEncode / MiniMaxAudioEncode -> SetLatentNoiseMask (x2) -> a concat node."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "video": ("VIDEO", {"tooltip": "Source video (mask editor or LoadVideo); its frames and audio track are encoded."}),
            "vae": ("VAE", {"tooltip": "Video VAE."}),
            "audio_vae": ("VAE", {"tooltip": "Audio VAE, e.g. the MiniMax H3 audio VAE."}),
            "mask": ("MASK", {"tooltip": "Video mask [F, H, W] per frame (1 = regenerate, 0 = keep)."}),
            "audio_mask": ("MASK", {"tooltip": "Audio mask [F] or [F, 1] at the video frame rate (1 = regenerate, 0 = keep)."}),
        }}

    RETURN_TYPES = ("LATENT",)
    RETURN_NAMES = ("latent",)
    FUNCTION = "encode"
    CATEGORY = "video"
    DESCRIPTION = ("Encodes a video's frames and audio into a nested AV latent with the video and audio masks attached "
                   "(1 = regenerate, 0 = keep).")

    def encode(self, video, vae, audio_vae, mask, audio_mask):
        NestedTensor = _nested_tensor()
        parts = video.get_components()
        z_video = vae.encode(parts.images[:, :, :, :3])
        if parts.audio is None:
            raise ValueError("the video has no audio track to encode")
        z_audio = LanPaint_MiniMaxAudioEncode().encode(parts.audio, audio_vae)[0]["samples"]
        return ({"samples": NestedTensor((z_video, z_audio)),
                 "noise_mask": NestedTensor((mask, _flat_audio_mask(audio_mask)))},)


class LanPaint_AVDecode:
    """Decodes a nested AV latent and merges it with the source video: frames inside the video mask (MaskBlend-style
    boundary of `blend_overlap` pixels, one lp_mask_blend launch), audio inside the audio mask (a box crossfade of
    `audio_crossfade` seconds, one lp_audio_merge job).  The result keeps the source's frame rate and bit depth; a source
    without an audio track gets the inpainted audio."""

    @classmethod
    def INPUT_TYPES(s):
        return {"required": {
            "samples": ("LATENT", {"tooltip": "Nested AV latent to decode (the sampler's output)."}),
            "video": ("VIDEO", {"tooltip": "Source video: the kept content, the frame rate and the bit depth."}),
            "vae": ("VAE", {"tooltip": "Video VAE."}),
            "audio_vae": ("VAE", {"tooltip": "Audio VAE, e.g. the MiniMax H3 audio VAE."}),
            "mask": ("MASK", {"tooltip": "Video mask [F, H, W] per frame (1 = regenerate, 0 = keep)."}),
            "audio_mask": ("MASK", {"tooltip": "Audio mask [F] or [F, 1] at the video frame rate (1 = regenerate, 0 = keep)."}),
            "blend_overlap": ("INT", {"default": 11, "min": 1, "max": 51, "step": 2,
                                      "tooltip": "Width in pixels of the blended boundary between inpainted and source frames."}),
            "audio_crossfade": ("FLOAT", {"default": 0.02, "min": 0.0, "max": 1.0, "step": 0.005,
                                          "tooltip": "Crossfade in seconds at the audio mask's edges (0 = hard cut)."}),
        }}

    RETURN_TYPES = ("VIDEO", "AUDIO")
    RETURN_NAMES = ("video", "audio")
    FUNCTION = "decode"
    CATEGORY = "video"
    DESCRIPTION = ("Decodes a nested AV latent, merges the inpainted video and audio into the source inside their masks, "
                   "and keeps the source's frame rate and bit depth.")

    def decode(self, samples, video, vae, audio_vae, mask, audio_mask, blend_overlap, audio_crossfade):
        VideoFromComponents, VideoComponents = _video_types()
        parts = video.get_components()
        src_frames, src_audio = parts.images, parts.audio
        z_video, z_audio = samples["samples"].unbind()

        frames = vae.decode(z_video)
        if frames.ndim == 5:                          # [1, F, H, W, C] from a video VAE: frames at batch
            frames = frames.reshape(-1, *frames.shape[-3:])
        decoded_audio = LanPaint_MiniMaxAudioDecode().decode({"samples": z_audio}, audio_vae)[0]

        size = (src_frames.shape[1], src_frames.shape[2])
        if tuple(frames.shape[1:3]) != size:          # VAE decodes can round the size
            frames = torch.nn.functional.interpolate(frames.movedim(-1, 1), size=size, mode="bilinear",
                                                     align_corners=False).movedim(1, -1)
        dev = node_device(src_frames)
        # the mask is handed over where it lives: its device decides the index rule of a lower-resolution mask's resample
        merged_frames = merge_video_with_mask(src_frames.to(dev), frames.to(dev), mask, blend_overlap).to(src_frames.device)

        merged_audio = decoded_audio
        if src_audio is not None:
            wave = src_audio["waveform"]
            merged = _audio.merge_audio_with_mask(wave.float(), decoded_audio["waveform"].float(), audio_mask,
                                                  audio_crossfade, src_audio["sample_rate"], decoded_audio["sample_rate"])
            merged_audio = {"waveform": merged.to(wave.device), "sample_rate": src_audio["sample_rate"]}

        out = VideoFromComponents(VideoComponents(images=merged_frames, audio=merged_audio, frame_rate=video.get_frame_rate()),
                                  bit_depth=video.get_bit_depth())
        return (out, merged_audio)


NODE_CLASS_MAPPINGS = {
    "LanPaint_MiniMaxAudioEncode": LanPaint_MiniMaxAudioEncode,
    "LanPaint_MiniMaxAudioDecode": LanPaint_MiniMaxAudioDecode,
    "LanPaint_AVEncode": LanPaint_AVEncode,
    "LanPaint_AVDecode": LanPaint_AVDecode,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LanPaint_MiniMaxAudioEncode": "LanPaint MiniMax Audio Encode",
    "LanPaint_MiniMaxAudioDecode": "LanPaint MiniMax Audio Decode",
    "LanPaint_AVEncode": "LanPaint AV Encode",
    "LanPaint_AVDecode": "LanPaint AV Decode",
}
