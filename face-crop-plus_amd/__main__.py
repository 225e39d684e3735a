"""Command line of the MI355X path: the reference's flags (``__main__.py:117-226``)
mapped one-to-one onto ``Cropper``; ``-c/--config`` JSON supplies defaults; negative
thresholds mean "disabled" (None).  ``python -m face_crop_plus_amd -i DIR``.

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m face_crop_plus_amd ...``;
rank 0 alone reads (or downloads) the checkpoints and broadcasts them over RCCL (weights.load_state_dict), then
each rank takes every N-th file batch (face_crop_plus_amd/dist.py) — no data-path collective.
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="face-crop-plus", description="Face crop / align / enhance / parse on MI355X")
    p.add_argument("-c", "--config", type=str, help="JSON file whose keys override the defaults below")
    p.add_argument("-i", "--input_dir", type=str, help="directory with input images")
    p.add_argument("-o", "--output-dir", type=str, default=None)
    p.add_argument("-cn", "--clean-names", action="store_true", help="copy the files to <input_dir>_temp under OS-safe names first (utils.clean_names)")
    p.add_argument("-ci", "--clean-names-inplace", action="store_true", help="rename the files to OS-safe names in place first")
    p.add_argument("-s", "--output-size", type=int, nargs="+", default=[256, 256])
    p.add_argument("-f", "--output-format", type=str, default=None)
    p.add_argument("-r", "--resize-size", type=int, nargs="+", default=[1024, 1024])
    p.add_argument("-ff", "--face-factor", type=float, default=0.65)
    p.add_argument("-st", "--strategy", type=str, default="largest")
    p.add_argument("-p", "--padding", type=str, default="constant")
    p.add_argument("-a", "--allow-skew", action="store_true")
    p.add_argument("-l", "--landmarks", type=str, default=None)
    p.add_argument("-ag", "--attr-groups", type=json.loads, default=None)
    p.add_argument("-mg", "--mask-groups", type=json.loads, default=None)
    p.add_argument("-dt", "--det-threshold", type=float, default=0.6)
    p.add_argument("-et", "--enh-threshold", type=float, default=-1)
    p.add_argument("-b", "--batch-size", type=int, default=8)
    p.add_argument("-n", "--num-processes", type=int, default=1)
    p.add_argument("-d", "--device", type=str, default="auto")
    # absent from the parsed arguments unless given, so that they stay exactly the reference parser's; Cropper's default
    # is "batch"
    p.add_argument("-cs", "--crop-source", type=str, default=argparse.SUPPRESS, choices=("batch", "original"),
                   help="sample crops from the resized batch (default 'batch', the reference's behaviour) or from the "
                        "full-resolution file ('original')")
    p.add_argument("-ip", "--interpolation", type=str, default=argparse.SUPPRESS, choices=("linear", "cubic", "lanczos4"),
                   help="filter of the crop warp: cv2 INTER_LINEAR (default 'linear', the reference's), INTER_CUBIC "
                        "('cubic') or INTER_LANCZOS4 ('lanczos4')")
    p.add_argument("-ms", "--min_sharpness", "--min-sharpness", type=float, default=argparse.SUPPRESS,
                   help="drop crops whose variance of the Laplacian (cv2.Laplacian(gray, cv2.CV_64F).var()) is below this "
                        "value; by default nothing is scored or dropped")
    p.add_argument("-enc", "--encoder", type=str, default=argparse.SUPPRESS, choices=("host", "device"),
                   help="where output files are compressed: 'host' (default, Pillow on the I/O pool) or 'device' (JPEG "
                        "files of aligned crops and masks are encoded on the GPU, byte for byte the same files)")
    p.add_argument("-penc", "--png-encoder", type=str, default=argparse.SUPPRESS, choices=("host", "device"),
                   help="where PNG files are compressed: 'host' (default, Pillow on the I/O pool) or 'device' (PNG files of "
                        "aligned crops and masks are filtered and deflated on the GPU: the same pixels, not the same bytes)")
    p.add_argument("-bg", "--background", type=_background, default=argparse.SUPPRESS,
                   help="replace the background of the crops with a uniform fill: 'R,G,B' or a single gray level, each "
                        "0..255; or 'transparent': RGBA cut-outs with the matte as their alpha channel (needs "
                        "--output-format png); by default the crops keep their background")
    p.add_argument("-fg", "--foreground", type=json.loads, default=argparse.SUPPRESS,
                   help="JSON list of the face parser's class indices that count as the subject (with --background; default "
                        "every class but 0)")
    p.add_argument("-fe", "--feather", type=int, default=argparse.SUPPRESS,
                   help="soft edge of the background replacement in pixels: 0, 3, 5 or 7 (with --background; default 5)")
    p.add_argument("-bb", "--background-blur", type=float, default=argparse.SUPPRESS,
                   help="keep the background of the crops and blur it: sigma in output pixels, 0.5..16, of a Gaussian over "
                        "the background pixels alone (not with --background; --foreground / --feather apply); by default "
                        "the crops keep their background")
    p.add_argument("-bi", "--background-image", type=str, nargs="+", metavar="PATH", default=argparse.SUPPRESS,
                   help="put the subject of the crops in front of a picture: image files and / or directories of them (not "
                        "with --background or --background-blur; --foreground / --feather apply); with several pictures a "
                        "face gets the one its output file name hashes to; by default the crops keep their background")
    p.add_argument("-bf", "--background-fit", type=str, default=argparse.SUPPRESS, choices=("cover", "stretch"),
                   help="how a picture of --background-image meets the output size: 'cover' (default) scales it uniformly "
                        "until it covers the crop and crops its centre, 'stretch' scales both axes on their own")
    p.add_argument("-rf", "--refine", type=int, default=argparse.SUPPRESS,
                   help="follow the image's edges with the matte: window radius in output pixels, 1..16, of a guided filter "
                        "of the mask (with --background or --background-blur, in place of --feather); by default the edge is "
                        "the feathered mask")
    p.add_argument("-re", "--refine-eps", type=int, default=argparse.SUPPRESS,
                   help="regulariser of --refine in gray levels squared, 1..4096 (default 64)")
    p.add_argument("-su", "--subject", choices=["largest"], default=argparse.SUPPRESS,
                   help="keep one connected subject in the matte: 'largest' keeps the largest 8-connected component of the "
                        "foreground, so other people and specks become background (with --background or --background-blur); "
                        "by default every foreground pixel counts")
    p.add_argument("-fh", "--fill-holes", type=int, default=argparse.SUPPRESS,
                   help="fill the matte's pinholes: the largest enclosed background region, in output pixels "
                        "(1..67108864), that becomes foreground (with --background or --background-blur); by default holes "
                        "stay")
    p.add_argument("-es", "--edge-shift", type=int, default=argparse.SUPPRESS,
                   help="grow (positive) or shrink (negative) the matte by this many output pixels, a non-zero int -64..64, "
                        "before its soft edge is made: -2 removes the ring of old background the parser leaves around the "
                        "subject (with --background or --background-blur); by default the boundary stays")
    p.add_argument("-dc", "--decontaminate", type=float, default=argparse.SUPPRESS,
                   help="give the soft edge of the matte the subject's own colour in place of its mix with the old "
                        "background: sigma in output pixels, 0.5..16, about the width of the soft edge or more (with "
                        "--background, fill or 'transparent'); by default the edge keeps the crop's colour")
    p.add_argument("-dn", "--denoise", type=float, default=argparse.SUPPRESS,
                   help="remove sensor noise from the crops: filter strength in gray levels, 1..32 (8 suits a small face "
                        "from a high-ISO photo), of a non-local-means filter; by default the crops keep their noise")
    p.add_argument("-cl", "--clahe", type=float, default=argparse.SUPPRESS,
                   help="equalise the contrast of the crops: clip limit (> 0, usually 2.0) of a contrast-limited adaptive "
                        "histogram equalisation of their luma; by default the crops keep their contrast")
    p.add_argument("-cg", "--clahe-grid", type=int, default=argparse.SUPPRESS,
                   help="tiles per side of the equalisation, 1..16 (with --clahe; default 8)")
    p.add_argument("-sh", "--sharpen", type=float, default=argparse.SUPPRESS,
                   help="sharpen the crops: amount, 0.05..4 (1.0 adds the whole difference), of an unsharp mask of their "
                        "gray, added to the three channels alike; by default the crops keep their softness")
    p.add_argument("-shs", "--sharpen-sigma", type=float, default=argparse.SUPPRESS,
                   help="sigma of the unsharp mask's blur in output pixels, 0.5..16 (with --sharpen; default 1.5)")
    p.add_argument("-sht", "--sharpen-threshold", type=int, default=argparse.SUPPRESS,
                   help="differences of up to this many gray levels, 0..255, are left alone (with --sharpen; default 0)")
    p.add_argument("-sk", "--smooth-skin", type=float, default=argparse.SUPPRESS,
                   help="smooth the skin and nothing else: range strength, 1..64 gray levels (10 suits a portrait), of a "
                        "bilateral filter over the pixels the face parser labels skin; by default the crops keep their skin")
    p.add_argument("-sks", "--smooth-sigma", type=float, default=argparse.SUPPRESS,
                   help="spatial sigma of the skin smoothing in output pixels, 0.5..8 (with --smooth-skin; default 3.0)")
    p.add_argument("-ska", "--smooth-amount", type=float, default=argparse.SUPPRESS,
                   help="how much of the smoothed skin replaces the crop's, 0.05..1 (with --smooth-skin; default 1.0)")
    p.add_argument("-skc", "--skin-classes", type=json.loads, default=argparse.SUPPRESS,
                   help="JSON list of the parser classes that count as skin (with --smooth-skin; default [1, 7, 8, 10, 14])")
    p.add_argument("-jq", "--jpeg-quality", type=int, default=argparse.SUPPRESS,
                   help="quality of the JPEG files written, 1..100 (default 95, cv2.imwrite's)")
    p.add_argument("-jss", "--jpeg-subsampling", type=str, default=argparse.SUPPRESS, choices=("4:4:4", "4:2:2", "4:2:0"),
                   help="chroma subsampling of the JPEG files written (default '4:2:0'; '4:4:4' keeps the colour at full "
                        "resolution)")
    p.add_argument("-jo", "--jpeg-optimize", action="store_true", default=argparse.SUPPRESS,
                   help="give every JPEG file Huffman tables of its own: smaller files, the same pixels")
    return p


def _background(text: str):
    """'R,G,B' -> [R, G, B], 'V' -> V, 'transparent' -> itself."""
    if text == "transparent":
        return text
    parts = [int(v) for v in text.split(",")]
    return parts[0] if len(parts) == 1 else parts


def parse_args(argv=None) -> dict:
    parser = build_parser()
    pre, _ = parser.parse_known_args(argv)
    if pre.config:
        with open(pre.config) as f:
            cfg = {k.replace("-", "_"): v for k, v in json.load(f).items()}
        parser.set_defaults(**cfg)
    args = vars(parser.parse_args(argv))
    args.pop("config")
    if args["input_dir"] is None:
        raise ValueError("Input directory must be specified.")        # __main__.py:231-232 of the reference
    for k in ("det_threshold", "enh_threshold"):
        if args[k] is not None and args[k] < 0:
            args[k] = None
    if args["device"] == "auto":
        args["device"] = f"cuda:{os.environ.get('LOCAL_RANK', '0')}"
    return args


def main(argv=None):
    kwargs = parse_args(argv)
    input_dir, output_dir = kwargs.pop("input_dir"), kwargs.pop("output_dir")
    needs_clean, is_inplace = kwargs.pop("clean_names"), kwargs.pop("clean_names_inplace")
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    temp_dir = None
    if needs_clean or is_inplace:                       # __main__.py:266-274 of the reference
        from .utils import clean_names
        if rank == 0:
            clean_names(input_dir=input_dir, output_dir=None if is_inplace else input_dir + "_temp")
        if needs_clean and not is_inplace:
            output_dir = input_dir + "_faces" if output_dir is None else output_dir
            input_dir = temp_dir = input_dir + "_temp"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        # RCCL ("nccl" IS RCCL on ROCm), one rank per GPU; FCP_DIST_BACKEND=gloo only for ranks that share a device (tests)
        dist.init_process_group(os.environ.get("FCP_DIST_BACKEND", "nccl"))
        dist.barrier()                                  # rank 0 has finished renaming / copying
    from .cropper import Cropper
    cropper = Cropper(**kwargs)
    cropper.process_dir(input_dir, output_dir)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if temp_dir is not None and rank == 0:
        import shutil
        shutil.rmtree(temp_dir)


if __name__ == "__main__":
    sys.exit(main())
