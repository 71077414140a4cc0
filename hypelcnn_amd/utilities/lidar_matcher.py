"""Where the GRSS2018 scene lies inside the GRSS2013 scene (reference utilities/lidar_matcher.py):

    python -m hypelcnn_amd.utilities.lidar_matcher --path <dir> --output_path <dir>

One band of each scene is brought to a common ground resolution by an integer enlargement (cv2.resize INTER_AREA, which
replicates pixels there), the template is laid over every position of the image and the position with the largest
normalised cross-correlation wins (cv2.matchTemplate TM_CCORR_NORMED, cv2.minMaxLoc).  All of it runs on the device
(common/device_match.py) without building the enlarged rasters; DESIGN §3.12 states the semantics, which are restated
from OpenCV's documentation and not pinned against cv2.  Defaults are the reference's: band 8 of GRSS2013 enlarged 5
times against band 2 of GRSS2018 without its last 350 rows and 75 columns, enlarged 2 times, both scenes normalised.
The other flags make it usable on other pairs.  Prints the reference's four lines and writes, under --output_path,

    lidar_match.json   score, corners in enlarged and in image pixels, geometry
    lidar_match.tif    uint8: the enlarged image band as grey levels with the matched rectangle framed in 255

The reference's two histogram plots (their bin edges degenerate on normalised data) and plt.show() are not reproduced;
the frame is drawn by slicing, not by cv2.rectangle's line rasteriser."""
import argparse
import json
import os

import numpy

from hypelcnn_amd.common import device_match as dm
from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers
from hypelcnn_amd.common.common_nn_ops import get_loader_from_name
from hypelcnn_amd.common.tiff_io import imwrite


def _crop(text):
    try:
        rows, cols = (int(v) for v in str(text).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--template_crop takes ROWS,COLS, not {text!r}") from None
    return rows, cols


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_loaders(parser)
    parser.add_argument("--image_loader", type=str, default="GRSS2013DataLoader", help="Loader of the searched scene")
    parser.add_argument("--template_loader", type=str, default="GRSS2018DataLoader", help="Loader of the located scene")
    parser.add_argument("--image_path", type=str, default=None, help="Data path of the image loader (default: --path)")
    parser.add_argument("--template_path", type=str, default=None,
                        help="Data path of the template loader (default: --path)")
    parser.add_argument("--image_band", type=int, default=8, help="Band of the image scene")
    parser.add_argument("--template_band", type=int, default=2, help="Band of the template scene")
    parser.add_argument("--image_scale", type=float, default=5, help="Integer enlargement of the image band")
    parser.add_argument("--template_scale", type=float, default=2, help="Integer enlargement of the template band")
    parser.add_argument("--template_crop", type=_crop, default=(350, 75),
                        help="ROWS,COLS dropped from the end of the template band")
    return parser


def _band(loader_name, path, band, backend, what):
    """-> (the band as a 2-D float32 raster: a view of the device scene where the loader prepared it there, else one
    band of the host scene; the scene's band count)"""
    loader = get_loader_from_name(loader_name, path)
    if hasattr(loader, "backend"):
        loader.backend = backend
    data_set = loader.load_data(0, True)
    scene = getattr(data_set, "casi_dev", None)
    if scene is None:
        scene = data_set.casi
    bands = int(scene.shape[2])
    if not 0 <= band < bands:
        raise ValueError(f"lidar_matcher: --{what}_band {band} is outside 0..{bands - 1}, the bands of {loader_name}")
    if isinstance(scene, numpy.ndarray):
        return numpy.ascontiguousarray(scene[:, :, band], dtype=numpy.float32), bands  # uploaded as one band
    return scene[:, :, band], bands  # read in place: sx = bands


def draw_frame(raster, top_left, bottom_right, width):
    """Sets a frame `width` pixels wide, centred on the edges of the rectangle and clipped to the raster, to 255."""
    h, w = raster.shape
    half = width // 2
    (x0, y0), (x1, y1) = top_left, bottom_right
    clip = lambda v, top: max(0, min(top, v))  # noqa: E731
    inner = (slice(clip(y0 + half, h), clip(y1 - half, h)), slice(clip(x0 + half, w), clip(x1 - half, w)))
    keep = raster[inner].copy()
    raster[clip(y0 - half, h):clip(y1 + half, h), clip(x0 - half, w):clip(x1 + half, w)] = 255
    raster[inner] = keep
    return raster


def main(argv=None, backend=None):
    """-> the dict written to lidar_match.json"""
    flags, _ = build_parser().parse_known_args(argv)
    if backend is None:
        from hypelcnn_amd.common.device_scene import resolve_scene_backend
        backend = resolve_scene_backend(None)
    if backend is None:
        from hypelcnn_amd.backend import HypelError
        raise HypelError("lidar_matcher runs on the compute device: no HIP device is visible "
                         "(there is no CPU fallback)")
    scales = {"image": dm._integer_scale(flags.image_scale, "image"),
              "template": dm._integer_scale(flags.template_scale, "template")}
    image, image_bands = _band(flags.image_loader, flags.image_path or flags.path, flags.image_band, backend, "image")
    template, template_bands = _band(flags.template_loader, flags.template_path or flags.path, flags.template_band,
                                     backend, "template")
    full_shape = tuple(int(v) for v in template.shape)
    rows, cols = flags.template_crop
    if rows < 0 or cols < 0 or rows >= full_shape[0] or cols >= full_shape[1]:
        raise ValueError(f"lidar_matcher: --template_crop {rows},{cols} leaves nothing of the "
                         f"{full_shape[0]} x {full_shape[1]} template band")
    template = template[:full_shape[0] - rows, :full_shape[1] - cols]

    image_band = dm._Band(backend, image, scales["image"], "image")
    template_band = dm._Band(backend, template, scales["template"], "template")
    found = dm.match_template(backend, image_band, template_band)
    scale = scales["image"]
    top_left, bottom_right = found.top_left, found.bottom_right
    print("Top Left", top_left)
    print("Top Left(scaled) (%f, %f)" % (top_left[0] / scale, top_left[1] / scale))
    print("Bottom Right", bottom_right)
    print("Bottom Right(scaled) (%f, %f)" % (bottom_right[0] / scale, bottom_right[1] / scale))

    figure = dm.render_u8(backend, image_band).cpu().numpy().reshape(image_band.H, image_band.W)
    draw_frame(figure, top_left, bottom_right, 4 * scale)
    result = {
        "score": found.score,
        "top_left": list(top_left), "bottom_right": list(bottom_right),
        "top_left_scaled": [v / scale for v in top_left], "bottom_right_scaled": [v / scale for v in bottom_right],
        "geometry": {
            "image": {"loader": flags.image_loader, "band": flags.image_band, "bands": image_bands,
                      "shape": [image_band.h, image_band.w], "scale": scale},
            "template": {"loader": flags.template_loader, "band": flags.template_band, "bands": template_bands,
                         "shape": [template_band.h, template_band.w], "scale": scales["template"],
                         "crop": [rows, cols]},
            "surface": list(found.shape),
        },
    }
    os.makedirs(flags.output_path, exist_ok=True)
    with open(os.path.join(flags.output_path, "lidar_match.json"), "w") as f:
        json.dump(result, f, indent=1)
    imwrite(os.path.join(flags.output_path, "lidar_match.tif"), figure)
    return result


if __name__ == "__main__":
    main()
