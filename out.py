"""Inference + save harness of the stitching path (re-statement of the reference's out.py:15-54,106-146,158-312,
SURVEY.md section 8 f-1 / f-3) on the MI355X package.

    python out.py --data_root_path ./demo/ --inf_cfg all_img1_with_inpaint_g12_transRef [--ckpt_path CKPT]

Same flags, `demo.txt` pair list (one directory per line holding input1.jpg / input2.jpg), RGB-float loading and
result-directory naming as the reference.  The forward (`type="test_out"`) and the TPS post-pipeline
(core/inference/tps_pipline.py, `stitch_amd.tps_pipeline`) run on the HIP kernels; the composition stage (out.py:277-312,
`cfg.use_composition`) runs on the post-TPS canvases.  The `mix_fn` plug-in named by `TPS_PIPELINE_CONFIG.mix_method` runs too
(`stitch_amd.mix_methods`).  Differences from the reference's files: the shipped configs name `transref_inpainter`, the TransRef
network on the GPU (`stitch_amd.transref`), whose module loads the reference's `400_Trans.pth` from
`stitch_amd/mix_methods/utils/TransRef/`; that checkpoint is not in the tree, and without it (or with the diffusion inpainter, out
of scope) a pass-through stands in, so with the shipped configs in
`warp2.jpg`, `mask2.jpg`, `ave_fusion.jpg`, `composition.jpg`, `learned_mask*.jpg` the thin border `mix_fn` leaves to the inpainter
is not synthesised (with `inpaint_all_area`: no hole is); `--inf_cfg all_img1_with_inpaint_g12_cv` / `inpaint_all_area_g12_cv`
select `cv_inpainter`, the reference's OpenCV Telea inpainter restated as GPU kernels (README.md; unpinned against OpenCV), which
fills them; with the shipped `tps_method="opencv"` the spline is this package's own pixel-unit TPS (OpenCV is not
installable here: unpinned against OpenCV).  `--multiband_fusion` adds an eleventh file of this package's own, `multiband_fusion.jpg`: the two
warped images blended over a Laplacian pyramid along their distance-transform seam (README.md, multiband_fusion); `--exposure_compensation
{gain,blocks}` equalises the two images' brightness from their overlap in front of that blend (README.md, exposure compensation); `--seam dp`
moves the blend's seam from the distance transforms' to a minimum-difference path through the overlap (README.md, seam_dp), `--seam gc` to a
minimum cut over the overlap (README.md, seam_gc); `--crop inner`
also writes `ave_fusion_crop.jpg` (and `multiband_fusion_crop.jpg`): the same canvases cut to the largest rectangle without a hole, found on
the GPU (README.md, inner_crop)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def get_config(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_root_path", type=str, default="./demo/")
    p.add_argument("--txt_file", type=str, default="demo.txt")
    p.add_argument("--result_dir", type=str, default="results")
    p.add_argument("--ckpt_path", "--restore_ckpt", dest="restore_ckpt", type=str, default="",
                   help="checkpoint (reference flag: --ckpt_path, out.py:18; --restore_ckpt kept as an alias); empty = random init")
    p.add_argument("--model_config_name", type=str, default="last_config")
    p.add_argument("--inf_cfg", type=str, default="all_img1_with_inpaint_g12_transRef")
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--skip_if_avg_fusion_exists", action="store_true")
    p.add_argument("--gpu_jpeg", action="store_true",
                   help="encode the result JPEGs on the GPU (the same files, byte for byte) instead of with Pillow on the host")
    p.add_argument("--jpeg_quality", type=int, default=None, metavar="N",
                   help="quality (1..100) of the result JPEGs, on either encoder; default: Pillow's 75")
    p.add_argument("--jpeg_subsampling", type=int, default=None, choices=(0, 1, 2),
                   help="chroma subsampling of the RGB result JPEGs: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (Pillow's default)")
    p.add_argument("--jpeg_optimize", action="store_true", help="write the result JPEGs with optimised Huffman tables (Pillow's optimize=True)")
    p.add_argument("--jpeg_restart_blocks", type=int, default=None, metavar="N",
                   help="restart interval of the result JPEGs in MCUs (Pillow's restart_marker_blocks), on either encoder")
    p.add_argument("--jpeg_restart_rows", type=int, default=None, metavar="N",
                   help="restart interval of the result JPEGs in MCU rows (Pillow's restart_marker_rows; wins over --jpeg_restart_blocks)")
    p.add_argument("--multiband_fusion", action="store_true",
                   help="also write multiband_fusion.jpg: the two warped images blended over a Laplacian pyramid along the distance-transform seam (GPU)")
    p.add_argument("--multiband_levels", type=int, default=None, metavar="N", help="pyramid levels of --multiband_fusion (0..16; default 5)")
    p.add_argument("--exposure_compensation", choices=("gain", "blocks"), default=None,
                   help="with --multiband_fusion: gain-compensate the two warped images from their overlap before the blend (one pair of gains, or one per tile)")
    p.add_argument("--exposure_block", type=int, default=None, metavar="N", help="tile side of --exposure_compensation (8, 16, 32 or 64; default 32)")
    p.add_argument("--seam", choices=("dp", "gc"), default=None,
                   help="with --multiband_fusion: blend along a minimum-difference seam through the overlap instead of the distance-transform seam (GPU): "
                        "dp a monotone path by dynamic programming, gc a minimum cut (push-relabel; synchronises with the host once per round)")
    p.add_argument("--crop", choices=("inner",), default=None,
                   help="also write ave_fusion_crop.jpg (and multiband_fusion_crop.jpg): the result cut to the largest rectangle inside the union of the two masks (GPU)")
    p.add_argument("--gpu_decode", action="store_true",
                   help="decode the input JPEGs on the GPU (Pillow's pixels, bit for bit); files outside the decoder's contract keep Pillow")
    p.add_argument("--dry-run", dest="dry_run", action="store_true",
                   help="list the pairs this rank would process (sharding rehearsal: no model, no GPU) and exit")
    args = p.parse_args(argv)
    if args.exposure_compensation is not None and not args.multiband_fusion:
        p.error("--exposure_compensation applies to the operands of --multiband_fusion: give that switch too")
    if args.seam is not None and not args.multiband_fusion:
        p.error("--seam decides the ownership of --multiband_fusion: give that switch too")
    if args.exposure_block is not None and args.exposure_compensation is None:
        p.error("--exposure_block needs --exposure_compensation")
    if args.exposure_block is not None and args.exposure_block not in (8, 16, 32, 64):
        p.error("--exposure_block must be 8, 16, 32 or 64")
    import stitch_amd
    cfg, tps = stitch_amd.load_inference_config(args.inf_cfg, args.model_config_name)
    for k, v in vars(args).items():
        if k in ("restore_ckpt", "gpu_jpeg", "gpu_decode", "jpeg_optimize", "multiband_fusion") and not v:         # (a switch that is off: config.txt stays what it was before the switch existed)
            continue
        if k in ("jpeg_quality", "jpeg_subsampling", "jpeg_restart_blocks", "jpeg_restart_rows", "multiband_levels", "exposure_compensation", "exposure_block", "seam", "crop") and v is None:
            continue
        cfg[k] = v
    cfg.TPS_PIPELINE_CONFIG = tps
    return cfg


def get_data_dict_list(data_root_path, txt_file):
    """out.py:106-123: one pair directory per line of the list file."""
    out = []
    with open(os.path.join(data_root_path, txt_file)) as f:
        for line in f:
            if line.strip():
                out.append({"DATA_PATH": os.path.join(data_root_path, line.strip()), "IMG1": "input1.jpg", "IMG2": "input2.jpg"})
    return out


def decodeSingleData(data_path, img1_name, img2_name):
    """host half of out.py:129-136 (cv2.imread + BGR->RGB there; PIL RGB decode here): two uint8 [H,W,3] arrays.  Runs on a
    prefetch thread one pair ahead of the GPU (PIL releases the GIL while decoding)."""
    from PIL import Image
    return tuple(np.ascontiguousarray(np.array(Image.open(os.path.join(data_path, name)).convert("RGB")).astype(np.uint8)[..., :3])
                 for name in (img1_name, img2_name))


class _JpegFile:
    """an input file as `readSingleData` leaves it: its bytes and the probe the GPU decoder needs"""
    __slots__ = ("path", "data", "info")

    def __init__(self, path, data, info):
        self.path, self.data, self.info = path, data, info


def readSingleData(data_path, img1_name, img2_name):
    """`decodeSingleData` with ``gpu_decode``: the worker thread only reads and probes the two files (`ops.jpeg_probe`), the pixels are
    made on the device by `uploadSingleData`.  A pair with a file the decoder does not take (progressive, restart intervals, other sampling
    factors, ...) goes through `decodeSingleData` unchanged, with one printed line."""
    import stitch_amd
    files = []
    for name in (img1_name, img2_name):
        path = os.path.join(data_path, name)
        with open(path, "rb") as f:
            data = f.read()
        info = stitch_amd.ops.jpeg_probe(data, restart=True)
        if info is None:
            print(f"gpu_decode: {data_path} decoded with Pillow ({name} is outside the GPU decoder's contract)", flush=True)
            return decodeSingleData(data_path, img1_name, img2_name)
        files.append(_JpegFile(path, data, info))
    return tuple(files)


def check_decode(statuses):
    """the status words of a pair's GPU decodes (read back here): a scan that does not hold its frame's blocks raises and names the file"""
    bad = [(path, int(st.item())) for path, st in statuses]
    bad = [(path, v) for path, v in bad if v]
    if bad:
        raise RuntimeError("gpu_decode: the scan of " + ", ".join(f"{p} (status {v})" for p, v in bad) + " does not hold the frame's blocks")


def uploadSingleData(arrays, resize_to_512=False, statuses=None):
    """device half of out.py:137-143: uint8 HWC -> float [1,3,H,W] in 0..255 on the GPU (`st_load_rgb8`, exact), optional 512 resize.
    A `_JpegFile` (``gpu_decode``) is decoded on the device first (`ops.jpeg_decode`; an L file tiled to three channels, as
    `.convert("RGB")` does); its status word goes to `statuses` as (path, device int32) for `check_decode`, or is checked here."""
    import stitch_amd
    ts = []
    for arr in arrays:
        if isinstance(arr, _JpegFile):
            px, st = stitch_amd.ops.jpeg_decode(arr.data, info=arr.info)
            if statuses is None:
                check_decode([(arr.path, st)])
            else:
                statuses.append((arr.path, st))
            u8 = (px if arr.info.ncomp == 3 else px.expand(-1, -1, 3).contiguous()).unsqueeze(0)
            hw = arr.info.H * arr.info.W
        else:
            u8 = torch.from_numpy(arr).unsqueeze(0).cuda(non_blocking=True)
            hw = arr.shape[0] * arr.shape[1]
        t = stitch_amd.ops.load_rgb8(u8) if hw % 4 == 0 else u8.permute(0, 3, 1, 2).float().contiguous()
        ts.append(stitch_amd.ops.resize_bilinear(t, 512, 512, False) if resize_to_512 else t)
    return ts[0], ts[1]


def loadSingleData(data_path, img1_name, img2_name, resize_to_512=False):
    """out.py:129-146 -> two float [1,3,H,W] tensors, 0..255 (host tensors, as the reference returns them)."""
    a, b = uploadSingleData(decodeSingleData(data_path, img1_name, img2_name), resize_to_512)
    return a.cpu(), b.cpu()


def to_pillow(t):
    from PIL import Image
    arr = t[0].detach().cpu().permute(1, 2, 0).clip(0, 255).to(torch.uint8).numpy()
    return Image.fromarray(arr)


def jpeg_params_of(cfg):
    """The `save` keywords the flags --jpeg_quality / --jpeg_subsampling / --jpeg_optimize / --jpeg_restart_blocks / --jpeg_restart_rows ask
    for; None when none is given."""
    kw = {k: getattr(cfg, "jpeg_" + k) for k in ("quality", "subsampling") if getattr(cfg, "jpeg_" + k, None) is not None}
    kw.update({"restart_marker_" + k: getattr(cfg, "jpeg_restart_" + k) for k in ("blocks", "rows") if getattr(cfg, "jpeg_restart_" + k, None) is not None})
    if getattr(cfg, "jpeg_optimize", False):
        kw["optimize"] = True
    return kw or None


def multiband_of(cfg):
    """The `multiband` argument the flags --multiband_fusion / --multiband_levels ask for: None without the switch, else the level count."""
    if not getattr(cfg, "multiband_fusion", False):
        return None
    levels = getattr(cfg, "multiband_levels", None)
    return 5 if levels is None else int(levels)


def exposure_of(cfg):
    """The `exposure` argument the flags --exposure_compensation / --exposure_block ask for: None without the switch, else (mode, block)."""
    mode = getattr(cfg, "exposure_compensation", None)
    if mode is None:
        return None
    block = getattr(cfg, "exposure_block", None)
    return mode, 32 if block is None else int(block)


def seam_of(cfg):
    """The `seam` argument the flag --seam asks for: None without it, else "dp" or "gc"."""
    return getattr(cfg, "seam", None)


def crop_of(cfg):
    """The `crop` argument the flag --crop asks for: None without it, else "inner"."""
    return getattr(cfg, "crop", None)


class _Saver:
    """JPEG writes of out.py:260-312.  The uint8 conversion runs on the GPU (clip + truncation, as `to_pillow_fn` does on the
    host), the bytes are copied to the host in the caller's thread, the JPEG encode + file write go to ``pool`` when one is given
    (``main``'s loop: the encoder releases the GIL, so the next pair's kernels are enqueued meanwhile).

    ``gpu_jpeg``: the same uint8 canvas is encoded on the device instead (`ops.jpeg_encode`, the file Pillow would write, byte for
    byte) on the caller's stream; nothing is read back until ``flush`` (the end of a pair), which reads the byte counts of all
    pending files together, copies exactly those bytes to the host in one transfer and hands the plain file writes to ``pool``.

    ``jpeg_params``: Pillow's `save` keywords ``quality``, ``subsampling``, ``optimize``, ``restart_marker_blocks``, ``restart_marker_rows`` for
    every file, on both paths (`jpeg_params_of`);
    ``subsampling`` is never passed for an L array."""

    def __init__(self, pool=None, gpu_jpeg=False, jpeg_params=None):
        self.pool, self.futures, self.gpu_jpeg = pool, [], gpu_jpeg
        self.pending = []
        self.jpeg_params = dict(jpeg_params or {})
        unknown = set(self.jpeg_params) - {"quality", "subsampling", "optimize", "restart_marker_blocks", "restart_marker_rows"}
        if unknown:
            raise ValueError(f"jpeg_params: unknown keys {sorted(unknown)}")

    def _keywords(self, ndim):
        return {k: v for k, v in self.jpeg_params.items() if not (k == "subsampling" and ndim == 2)}

    def _write(self, arr, path):
        from PIL import Image
        Image.fromarray(arr).save(path, **self._keywords(arr.ndim))

    @staticmethod
    def _write_bytes(data, path):
        with open(path, "wb") as f:
            f.write(data)

    def _submit(self, fn, *args):
        if self.pool is None:
            fn(*args)
        else:
            self.futures.append(self.pool.submit(fn, *args))

    def image(self, t, path):
        u8 = t[0].detach().clip(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        self.array(u8, path)

    def array(self, arr, path):
        """uint8 [H,W,3] / [H,W], a device tensor or a host array"""
        if self.gpu_jpeg:
            import stitch_amd
            if not torch.is_tensor(arr):
                arr = torch.from_numpy(arr)
            self.pending.append(stitch_amd.ops.jpeg_encode(arr.cuda(), **self._keywords(arr.dim())) + (path,))
            return
        if torch.is_tensor(arr):
            arr = arr.cpu().numpy()
        self._submit(self._write, arr, path)

    def flush(self):
        """gpu_jpeg: device -> host of the files queued so far, on the current stream: the counts together, then exactly those bytes
        in one transfer; the file writes go to the pool.  (Deferring the read-back until the next pair's graph had been enqueued was
        measured slower at depth 3, 59 against 68 pairs/s, and no faster at depth 2: README.md.)"""
        if not self.pending:
            return
        files, self.pending = self.pending, []
        counts = torch.cat([n for _, n, _ in files]).tolist()
        data = torch.cat([buf[:c] for (buf, _, _), c in zip(files, counts)]).cpu().numpy()
        at = 0
        for (_, _, path), c in zip(files, counts):
            self._submit(self._write_bytes, data[at:at + c].tobytes(), path)
            at += c

    def wait(self):
        self.flush()
        for f in self.futures:
            f.result()
        self.futures = []


@torch.no_grad()
def load_inpainter(name):
    """out.py:341-346: `core.inference.mix_methods.utils.<name>.inpainter`.  `cv_inpainter` (the reference's OpenCV Telea
    inpainter, GPU kernels here) is shipped; `transref_inpainter` (the TransRef network, GPU kernels) is shipped but its module needs
    the reference's checkpoint `mix_methods/utils/TransRef/400_Trans.pth` and raises ImportError without it; the diffusion inpainter
    is out of scope.  `patchmatch_inpainter` (exemplar hole filling on the GPU, no weights, no counterpart in the reference;
    `inf_configs/*_pm.py`) is shipped too.  A module that cannot be imported falls back to the pass-through stand-in."""
    import importlib
    try:
        return importlib.import_module(f"stitch_amd.mix_methods.utils.{name}").inpainter
    except ImportError:
        print(f"[out.py] inpainter {name!r} is not available here (out of scope): using the pass-through stand-in -- holes keep "
              f"what mix_fn fills from image 1, the thin border it leaves to the inpainter stays as is")
        return importlib.import_module("stitch_amd.mix_methods.utils.passthrough_inpainter").inpainter


def inference_one_data(cfg, data_dict, save_root_path, warp_model, composition_model=None, inpainter=None, forward=None, saver=None,
                       gpu_jpeg=False, gpu_decode=False, jpeg_params=None, multiband=None, exposure=None, seam=None, crop=None):
    """out.py:158-312: forward (`test_out`), TPS post-pipeline with the configured `mix_fn`, saves, composition.  The inpainter
    is the caller's, else the pass-through stand-in (`load_inpainter`: `transref_inpainter` needs its checkpoint, the diffusion one is
    out of scope): with the stand-in, in `warp2.jpg`, `mask2.jpg`, `ave_fusion.jpg` and the
    composition inputs the holes hold what `mix_fn` fills from image 1 and the thin border region it hands to the inpainter is not
    synthesised; `cv_inpainter` (GPU Telea inpainting, unpinned against OpenCV) fills it, and `patchmatch_inpainter` (GPU exemplar
    fill, this project's own contract, pinned against no library) fills it with image content instead of diffused border colours.

    ``forward``: a callable returning the `test_out` dict of this pair whose network part is already in flight (``main``
    launches pair i + 1's hipGraph before it finishes pair i); default = load + ``warp_model(..., type="test_out")`` here.
    ``saver``: a ``_Saver`` (JPEG encodes on a thread pool); default = write synchronously, with ``gpu_jpeg`` through the device encoder.
    ``gpu_decode``: the two input files are decoded on the device (`readSingleData`, `ops.jpeg_decode`) when this function loads them.
    ``jpeg_params``: the `save` keywords of the default saver (`_Saver`); a caller's ``saver`` carries its own.
    ``multiband``: None, or the pyramid levels of an eleventh file `multiband_fusion.jpg` written after `ave_fusion.jpg`: `output1` and
    `output2` blended by `ops.multiband_blend` under `mask1` / `mask2`, as they go to the saver (README.md, multiband_fusion); the blend is
    returned as `multiband_image`.  This file is the package's own, not one of the reference's.
    ``exposure``: None, or (mode, block) of `ops.exposure_compensate`, applied to the two operands of that blend and to nothing else (needs
    ``multiband``); the compensated pair is returned as `compensated1` / `compensated2`.
    ``seam``: None, "dp" or "gc": `ops.seam_dp` / `ops.seam_gc` on the operands of that blend (the compensated pair when there is one) decides
    the ownership of the overlap (needs ``multiband``); its planes are returned as `seam_side` / `seam_info`.  "gc" reads its status record
    back from the device once per round (README.md, seam_gc).
    ``crop``: None, or "inner": `ops.inner_rect` on `mask1` / `mask2` as they go to the saver finds the largest rectangle inside their union
    (README.md, inner_crop); `ave_fusion_crop.jpg` (and, with ``multiband``, `multiband_fusion_crop.jpg`) is that slice of the uncropped
    canvas through the same saver.  The rectangle is searched directly after `ave_fusion.jpg` is queued, but the slice's size is data, so
    the six ints are read back once per pair, after all of the pair's other launches are enqueued; the crop files are queued then, the
    cropped `ave_fusion` first (before the saver's flush, so ``gpu_jpeg`` reads them back with the others), and none is written when the
    union is empty.  Returned as `crop_info` (device int32 [6]) and `crop_rect` (host (top, left, h, w), or None).  The composition network's
    files are not cropped: its canvas may be resized, so the rectangle does not apply to them."""
    if crop not in (None, "inner"):
        raise ValueError(f'crop must be None or "inner", got {crop!r}')
    if exposure is not None and multiband is None:
        raise ValueError("exposure compensation applies to the operands of the multiband blend: multiband must be given")
    if seam not in (None, "dp", "gc"):
        raise ValueError(f'seam must be None, "dp" or "gc", got {seam!r}')
    if seam is not None and multiband is None:
        raise ValueError("the seam decides the ownership of the multiband blend: multiband must be given")
    own_saver = saver is None
    statuses = []
    saver = saver or _Saver(gpu_jpeg=gpu_jpeg, jpeg_params=jpeg_params)
    path = data_dict["DATA_PATH"]
    name = os.path.basename(os.path.normpath(path))
    result_path = os.path.join(save_root_path, name) + "/"
    os.makedirs(result_path, exist_ok=True)
    if forward is not None:
        out = forward()
    else:
        image1, image2 = uploadSingleData((readSingleData if gpu_decode else decodeSingleData)(path if path.endswith("/") else path + "/", data_dict["IMG1"],
                                                                                              data_dict["IMG2"]),
                                          resize_to_512=cfg.resize_to_512, statuses=statuses)
        if getattr(cfg, "swap_image", False):
            image1, image2 = image2, image1
        out = warp_model(image1, image2, type="test_out", pad_mode=cfg.pad_mode)
    if inpainter is None:
        inpainter = load_inpainter(getattr(cfg.TPS_PIPELINE_CONFIG, "inpainter", "") or "passthrough_inpainter")
    # ---- TPS post-pipeline incl. the mix_fn plug-in (out.py:218-258, core/inference/tps_pipline.py:20-205) on the GPU
    import stitch_amd
    tpc = cfg.TPS_PIPELINE_CONFIG
    fb = getattr(cfg, "use_fb_consistency_mask", False) and "occlusion_mask" in out     # (flow_source="zero" computes no flow, so no consistency mask either)
    occlusion_mask = out.get("occlusion_mask")
    if occlusion_mask is None:
        # no flow, nothing occluded: the mask the consistency check gives for a zero backward flow, all ones on image 1's footprint on the canvas
        ones = torch.ones((1, 1) + tuple(out["residual_flow"].shape[2:]), device=out["output1"].device)
        occlusion_mask = stitch_amd.ops.homo_warp(ones, out["I_mat"].view(1, 9), (out["out_height"], out["out_width"]))
    valid = out["origin_occlusion_mask"] if (fb and tpc.use_valid_on_flow) else None                      # out.py:219-222
    border_points_mask = None
    if fb and tpc.use_border_points_mask:                                                                 # out.py:224-232
        border_points_mask = out["occlusion_mask"] if tpc.use_occ_filter else (out["H_warp_mask"].mean(dim=1, keepdim=True) > 0.5).float()
    inputs = dict(output1=out["output1"], mask1=out["mask1"], H_warp=out["H_warp"], H_warp_mask=out["H_warp_mask"],
                  final_warp=out["final_warp"], mask2=out["mask2"], residual_flow=out["residual_flow"], valid=valid,
                  occlusion_mask=occlusion_mask, border_points_mask=border_points_mask)
    limit = dict(width_min=out["width_min"], height_min=out["height_min"], out_height=out["out_height"], out_width=out["out_width"])
    import importlib
    mix_fn = importlib.import_module(f"stitch_amd.mix_methods.{tpc.mix_method}").mix_fn                     # out.py:235
    inpaint_fn = lambda **kw: mix_fn(**kw, inpainter=inpainter, use_composition=tpc.use_composition_when_inpaint,   # noqa: E731
                                     is_plot=tpc.is_plot, resize_to_area_limit_before_inpaint=tpc.resize_to_area_limit_before_inpaint)
    new = stitch_amd.tps_pipeline.tps_H_warp(inputs, limit, tpc, inpaint_fn=inpaint_fn)
    out = dict(out, forward_output2=out["output2"], forward_mask2=out["mask2"], forward_blend_image=out["blend_image"],
               new_blend_image=new["new_blend_image"], tps_output=new["tps_output"], output2=new["output2"],
               mask2=new["mask2"] if new["mask2"].shape[1] == 3 else new["mask2"].expand(-1, 3, -1, -1))   # 1 channel normally; the
    #                      mix_fn branch "inpaint result all zero: not used" returns a 3-channel mask (reference: passed through as is)
    saver.image(out["H_warp"], result_path + "H_warp.jpg")
    saver.image(out["final_warp"], result_path + "flow_warp.jpg")
    saver.image(out["output1"], result_path + "warp1.jpg")
    saver.image(out["output2"], result_path + "warp2.jpg")                                                # out.py:265-272
    for key in ("mask1", "mask2"):
        saver.array((out[key] > 0.5)[0, 0].to(torch.uint8).mul(255), result_path + key + ".jpg")
    saver.image(out["new_blend_image"].float(), result_path + "ave_fusion.jpg")
    if crop is not None:
        out = dict(out, crop_info=stitch_amd.ops.inner_rect(out["mask1"].float(), out["mask2"].float()))
    if multiband is not None:
        img1, img2, k1, k2 = out["output1"].float().contiguous(), out["output2"].float().contiguous(), out["mask1"].float(), out["mask2"].float()
        if exposure is not None:
            img1, img2 = stitch_amd.ops.exposure_compensate(img1, img2, k1, k2, mode=exposure[0], block=exposure[1])
            out = dict(out, compensated1=img1, compensated2=img2)
        pair = None
        if seam is not None:
            pair = (stitch_amd.ops.seam_gc if seam == "gc" else stitch_amd.ops.seam_dp)(img1, img2, k1, k2)
            out = dict(out, seam_side=pair[0], seam_info=pair[1])
        out = dict(out, multiband_image=stitch_amd.ops.multiband_blend(img1, img2, k1, k2, levels=multiband, seam=pair))
        saver.image(out["multiband_image"], result_path + "multiband_fusion.jpg")
    if composition_model is not None:
        # out.py:277-312: learned seam masks + composed image from the UDIS2 composition network
        mask1, mask2 = (out["mask1"] > 0.5).float(), (out["mask2"] > 0.5).float()
        comp = stitch_amd.composition.compose(composition_model, out["output1"], out["output2"], mask1, mask2)
        saver.image((comp["stitched_image"] + 1) * 127.5, result_path + "composition.jpg")
        for key in ("learned_mask1", "learned_mask2"):
            saver.image(comp[key] * 255, result_path + key + ".jpg")
        out = dict(out, **comp)
    if crop is not None:
        valid, top, left, h, w, _ = out["crop_info"].tolist()          # the one read of the pair: everything else is enqueued
        out = dict(out, crop_rect=(top, left, h, w) if valid else None)
        if valid:
            saver.image(out["new_blend_image"].float()[..., top:top + h, left:left + w], result_path + "ave_fusion_crop.jpg")
            if multiband is not None:
                saver.image(out["multiband_image"][..., top:top + h, left:left + w], result_path + "multiband_fusion_crop.jpg")
    saver.flush()
    check_decode(statuses)
    if own_saver:
        saver.wait()
    return out, result_path


def run_pairs(cfg, todo, save_root, model, composition_model=None, inpainter=None, on_done=None, depth=2, gpu_jpeg=False, gpu_decode=False,
              jpeg_params=None, multiband=None, exposure=None, seam=None, crop=None):
    """The inference loop of out.py:351-357 as a software pipeline, `depth` pairs in flight.  While pair i is finished on the host
    (canvas bounds read back, canvas kernels, TPS post-pipeline with its control-point round trips, composition, device->host copies
    of the images), the network parts of pairs i + 1 .. i + depth - 1 -- both nets at 512x512, ~1 000 launches each, replayed from a
    hipGraph (`GraphedTestOut.launch`) -- are already running on their own HIP streams, the JPEGs of the pairs after them are being
    decoded, and pair i - 1's JPEGs are being encoded, both on worker threads.  `depth` graph objects alternate so that a pair's static
    buffers (`residual_flow`, ...) are not overwritten before its post-pipeline has consumed them.  Same kernels and the same files
    as calling `inference_one_data` pair by pair (tests/test_harness_gpu.py).  Measured on 48 synthetic 512x512 pairs, 10 JPEGs written per
    pair (tools/bench_out_harness.py, profiles/r4_out_harness.json): 36.9 pairs/s pair by pair, 60.0 at depth 2 (default), 51 at depth 3 / 4
    (a third network graph in flight only delays the canvas / TPS / composition kernels of the pair the host is waiting for).
    ``gpu_jpeg``: the ten files of a pair are encoded on the device on the pair's stream (`_Saver(gpu_jpeg=True)`) and read back, counts
    first, at the end of the pair; the pool then only writes files.
    ``gpu_decode``: the decode threads only read and probe the files (`readSingleData`), the pixels are made on the pair's stream
    (`ops.jpeg_decode`) in front of its graph launch; the status words are checked when the pair is finished.
    ``jpeg_params``: Pillow's `save` keywords for the result files (`_Saver`), on either encoder.
    ``multiband``: the pyramid levels of `multiband_fusion.jpg` (`inference_one_data`), blended on the pair's stream; None: not written.
    ``exposure``: (mode, block) of the gain compensation in front of that blend (`inference_one_data`); None: none.
    ``seam``: "dp" for that blend along the minimum-difference path, "gc" along the minimum cut (`inference_one_data`); None: the distance seam.
    ``crop``: "inner" to write `ave_fusion_crop.jpg` / `multiband_fusion_crop.jpg` too (`inference_one_data`: one six-int read per pair); None: not written."""
    from concurrent.futures import ThreadPoolExecutor
    if not todo:
        return []
    depth = max(1, int(depth))
    graphs = [model.graphed_test_out() for _ in range(depth)]
    streams = [torch.cuda.Stream() for _ in range(depth)]
    done = []
    with ThreadPoolExecutor(max_workers=2) as dec_pool, ThreadPoolExecutor(max_workers=4) as enc_pool:
        def decode(dd):
            p = dd["DATA_PATH"]
            return (readSingleData if gpu_decode else decodeSingleData)(p if p.endswith("/") else p + "/", dd["IMG1"], dd["IMG2"])

        decoded = [dec_pool.submit(decode, dd) for dd in todo[:depth + 1]]

        def launch(j):
            k = j % depth
            arrays = decoded[j].result()
            decoded[j] = None                  # the Future keeps both uint8 arrays alive: release it (the reference's loop holds one pair)
            if j + depth + 1 < len(todo):
                decoded.append(dec_pool.submit(decode, todo[j + depth + 1]))
            statuses = []
            with torch.cuda.stream(streams[k]):
                image1, image2 = uploadSingleData(arrays, resize_to_512=cfg.resize_to_512, statuses=statuses)
                if getattr(cfg, "swap_image", False):
                    image1, image2 = image2, image1
                return graphs[k], graphs[k].launch(image1, image2), streams[k], statuses

        inflight = [launch(j) for j in range(min(depth - 1, len(todo)))]
        saver = _Saver(enc_pool, gpu_jpeg=gpu_jpeg, jpeg_params=jpeg_params)
        for j, dd in enumerate(todo):
            if j + depth - 1 < len(todo):
                inflight.append(launch(j + depth - 1))
            g, handle, st, statuses = inflight.pop(0)
            with torch.cuda.stream(st):
                out, rp = inference_one_data(cfg, dd, save_root, model, composition_model, inpainter,
                                             forward=lambda: g.finish(handle), saver=saver, multiband=multiband, exposure=exposure, seam=seam, crop=crop)
                check_decode(statuses)
            # no host wait here: the graph of this slot is launched again on the SAME stream (pair j + depth), i.e. after everything
            # that reads this pair's static buffers
            print("saved", rp)
            done.append(rp)
            if on_done is not None:
                on_done(j, out)
        saver.wait()
    return done


def shard_of_this_rank(data, rank, world):
    """Pairs are independent: under ``torchrun --nproc-per-node N out.py ...`` rank r takes pairs r, r + N, ... of the list
    (`stitch_amd.dist.shard_indices`; replaces the reference's single-process nn.DataParallel, out.py:80) and every rank
    writes its own result directories; no collective is needed."""
    from stitch_amd import dist as sdist
    return [data[i] for i in sdist.shard_indices(len(data), rank, world)]


def main(argv=None):
    import stitch_amd
    from stitch_amd import dist as sdist
    cfg = get_config(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if getattr(cfg, "dry_run", False):
        rank = int(os.environ.get("RANK", "0"))
        mine = shard_of_this_rank(get_data_dict_list(cfg.data_root_path, cfg.txt_file), rank, world)
        print("DRY_RUN rank", rank, "of", world, "pairs", [os.path.basename(os.path.normpath(d["DATA_PATH"])) for d in mine], flush=True)
        return None
    if world > 1:
        rank, world, local = sdist.init()              # one process per GPU: binds this process to cuda:LOCAL_RANK
    else:
        rank, local = 0, cfg.gpu
        torch.cuda.set_device(cfg.gpu)
    model = stitch_amd.build_model(cfg)
    if cfg.restore_ckpt:
        model.load_state_dict(torch.load(cfg.restore_ckpt, map_location="cpu", weights_only=True), strict=True)
    else:
        print("[out.py] no --restore_ckpt given: running with random-init weights (plumbing only)")
    model = model.cuda().eval()
    composition_model = None
    if getattr(cfg, "use_composition", False):
        import stitch_amd
        path = getattr(cfg, "composition_model_path", "")
        if path and os.path.exists(path):
            composition_model, _ = stitch_amd.composition.load_com_model(path)                 # out.py:95-103
        else:
            print(f"[out.py] composition checkpoint {path!r} not found: random-init composition network (plumbing only)")
            composition_model = stitch_amd.composition.Network().cuda().eval()
    inpainter = load_inpainter(getattr(cfg.TPS_PIPELINE_CONFIG, "inpainter", "") or "passthrough_inpainter")   # out.py:339-346
    model_name = cfg.restore_ckpt.split("/")[-2] if cfg.restore_ckpt.count("/") >= 1 else "random"
    tag = "512" if cfg.resize_to_512 else ""
    tps = cfg.TPS_PIPELINE_CONFIG
    suffix = f"{tag}_{model_name}_{tps.get_pt_methods[0]}_{tps.mix_method}_g{tps.grid_h}"
    save_root = os.path.abspath(os.path.join(cfg.data_root_path, f"../{cfg.result_dir}/")) + f"/ours_{suffix}/"
    os.makedirs(save_root, exist_ok=True)
    with open(save_root + "config.txt", "w") as f:
        f.write(repr(dict(cfg)))
    todo = []
    for dd in shard_of_this_rank(get_data_dict_list(cfg.data_root_path, cfg.txt_file), rank, world):
        if cfg.skip_if_avg_fusion_exists and os.path.exists(os.path.join(save_root, os.path.basename(os.path.normpath(dd["DATA_PATH"])), "ave_fusion.jpg")):
            print("[WARNING] Skip, Due to exist", dd["DATA_PATH"])
            continue
        todo.append(dd)
    run_pairs(cfg, todo, save_root, model, composition_model, inpainter, gpu_jpeg=bool(getattr(cfg, "gpu_jpeg", False)),
              gpu_decode=bool(getattr(cfg, "gpu_decode", False)), jpeg_params=jpeg_params_of(cfg), multiband=multiband_of(cfg), exposure=exposure_of(cfg),
              seam=seam_of(cfg), crop=crop_of(cfg))
    if world > 1:
        import torch.distributed as tdist
        tdist.barrier()
        tdist.destroy_process_group()
    return save_root


if __name__ == "__main__":
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import stitch_amd                                   # noqa: F401
        from stitch_amd import dist as _sdist
        with _sdist.rank_guard("out.py"):
            main()
    else:
        main()
