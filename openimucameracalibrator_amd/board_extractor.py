"""Checkerboard corner extraction: host-side mirror of the reference's core::BoardExtractor (src/core/board_extractor.cc)
and applications/extract_board_to_json.cc for the radon marker board, over the C-ABI entry oicc_board_radon_detect.
Resize, gray conversion, corner response, candidate selection, sub-pixel refinement and the marker check run on the
MI355X; grid assembly runs on the host inside the library.  There is no CPU fallback.  Charuco and AprilTag boards and
video input are not supported ("Board extraction")."""
import argparse
import ctypes as C
import glob
import os
import sys

import numpy as np

from . import _abi
from . import _lib
from . import io_files

CHARUCO, RADON, APRILTAG = 0, 1, 2          # BoardType (include/OpenCameraCalibrator/core/board_extractor.h:30-35)
BOARD_TYPES = {"charuco": CHARUCO, "radon": RADON, "apriltag": APRILTAG}
DEFAULT_OPTIONS = dict(radius=3, threshold_rel=0.5, max_candidates=512, subpix_iterations=20, subpix_eps=0.01, batch=64)
NS_TO_S, S_TO_US = 1e-9, 1e6                # utils/types.h:29-33


def radon_detect(frames, downsample_factor, W, H, device=0, stages=False, **options):
    """oicc_board_radon_detect on frames [F, h, w] (gray) or [F, h, w, 3] (BGR) u8.  Returns corners [F, W*H, 2] (NaN
    where not found), found [F] bool, candidates per frame, the report dict, and with stages=True also the gray and
    blurred images, the response and polarity maps, the per-frame candidate / refined lists (raster order), and per frame
    the assembled grid of candidate indices [A, B] with its disc / ring means [A-1, B-1] (None without a grid) and
    grid_shape [F, 2] ((0, 0) without a grid)."""
    b = _lib.load_board()
    fr = np.ascontiguousarray(np.asarray(frames, dtype=np.uint8))
    if fr.ndim not in (3, 4) or (fr.ndim == 4 and fr.shape[3] != 3):
        raise ValueError("frames must be [F, h, w] or [F, h, w, 3] u8")
    F, h, w = fr.shape[:3]
    ch = 1 if fr.ndim == 3 else 3
    o = dict(DEFAULT_OPTIONS, **options)
    opt = _abi.BoardOptions(int(o["radius"]), float(o["threshold_rel"]), int(o["max_candidates"]), int(o["subpix_iterations"]),
                            float(o["subpix_eps"]), int(o["batch"]), 0)
    corners = np.zeros((F, W * H, 2), np.float64)
    found = np.zeros(F, np.int32)
    ncand = np.zeros(F, np.int32)
    rep = _abi.BoardReport()
    st = None
    if stages:
        wd, hd = C.c_int32(), C.c_int32()
        if b.output_size(w, h, float(downsample_factor), C.byref(wd), C.byref(hd)) != 0:
            raise ValueError("bad image size or downsample factor")
        cap = int(o["max_candidates"])
        gray = np.zeros((F, hd.value, wd.value), np.uint8)
        resp = np.zeros((F, hd.value, wd.value), np.float32)
        cxy = np.zeros((F, cap, 2), np.int32)
        ref = np.zeros((F, cap, 2), np.float64)
        pol = np.zeros((F, hd.value, wd.value), np.uint8)
        blur = np.zeros((F, hd.value, wd.value), np.float32)
        gshape = np.zeros((F, 2), np.int32)
        grid = np.zeros((F, W * H), np.int32)
        disc = np.zeros((F, (W - 1) * (H - 1)), np.float64)
        ring = np.zeros((F, (W - 1) * (H - 1)), np.float64)
        st = _abi.BoardStages(gray.ctypes.data_as(_abi.c_u8p), resp.ctypes.data_as(C.POINTER(C.c_float)), cxy.ctypes.data_as(_abi.c_i32p),
                              ref.ctypes.data_as(_abi.c_dp), cap, 1, pol.ctypes.data_as(_abi.c_u8p), blur.ctypes.data_as(C.POINTER(C.c_float)),
                              gshape.ctypes.data_as(_abi.c_i32p), grid.ctypes.data_as(_abi.c_i32p), disc.ctypes.data_as(_abi.c_dp),
                              ring.ctypes.data_as(_abi.c_dp))
    rc = b.radon_detect(int(device), F, w, h, ch, fr.ctypes.data_as(_abi.c_u8p), float(downsample_factor), int(W), int(H), C.byref(opt),
                        corners.ctypes.data_as(_abi.c_dp), found.ctypes.data_as(_abi.c_i32p), ncand.ctypes.data_as(_abi.c_i32p),
                        C.byref(rep), C.byref(st) if st is not None else None)
    if rc != 0:
        raise RuntimeError("oicc_board_radon_detect failed (%d)" % rc)
    out = (corners, found.astype(bool), ncand, rep.as_dict())
    if stages:
        n = np.minimum(ncand, cap)
        has = [bool(gshape[f, 0]) for f in range(F)]
        cells = lambda a, f: a[f].reshape(gshape[f, 0] - 1, gshape[f, 1] - 1).copy() if has[f] else None
        out += (dict(gray=gray, response=resp, candidates=[cxy[f, :n[f], ::-1].copy() for f in range(F)],
                     refined=[ref[f, :n[f]].copy() for f in range(F)], polarity=pol, blurred=blur, grid_shape=gshape,
                     grid=[grid[f].reshape(gshape[f]).copy() if has[f] else None for f in range(F)],
                     disc=[cells(disc, f) for f in range(F)], ring=[cells(ring, f) for f in range(F)]),)
    return out


def read_png_bgr(path):
    """cv::imread(path) (IMREAD_COLOR) for 8-bit PNGs: [h, w, 3] BGR, or [h, w] when the file is gray (its BGR
    conversion gives back the same gray values, so the gray path is taken directly)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("L", "LA"):
            return np.asarray(im.convert("L"), dtype=np.uint8)
        if im.mode not in ("RGB", "RGBA"):
            raise ValueError("%s: unsupported PNG mode %s (8-bit gray, gray + alpha, RGB or RGBA)" % (path, im.mode))
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])


def timestamp_ns_of(path):
    """std::stoul of the file name (board_extractor.cc:305-309): its leading digits."""
    stem = os.path.basename(path)
    digits = stem[:len(stem) - len(stem.lstrip("0123456789"))]
    if not digits:
        raise ValueError("file name is not a timestamp in ns: %s" % path)
    return int(digits)


def view_key(t_s):
    """std::to_string(timestamp_s * S_TO_US) (board_extractor.cc:314): %f, six decimals."""
    return "%f" % (t_s * S_TO_US)


def median_of_doubles(v):
    """utils::MedianOfDoubleVec (src/utils/utils.cc:77-97)."""
    v = sorted(v)
    n = len(v)
    return (v[n // 2 - 1] + v[n // 2]) / 2 if n % 2 == 0 else v[n // 2]


def camera_fps(times_s):
    """board_extractor.cc:367-375: the timestamps as a std::set, deltas for i < size() - 2 (the last delta is dropped),
    1 / median."""
    t = sorted(set(times_s))
    if len(t) < 3:
        raise ValueError("at least three frames are needed for camera_fps (board_extractor.cc:371 reads size() - 2)")
    return 1.0 / median_of_doubles([t[i + 1] - t[i] for i in range(len(t) - 2)])


class BoardExtractor:
    """core::BoardExtractor (board_extractor.h:48-140) for BoardType::RADON."""

    def __init__(self, device=0, **options):
        self.device = device
        self.options = dict(DEFAULT_OPTIONS, **options)
        self.board_initialized_ = False
        self.verbose_plot_ = False
        self.report = {}

    def SetVerbosePlot(self):
        self.verbose_plot_ = True          # the reference shows an OpenCV window; here a per-batch line is printed

    def InitializeRadonBoard(self, square_length, squaresX, squaresY):
        """board_extractor.cc:73-93: W x H inner corners, id i*W + j, board point ((float)i * s, (float)j * s, 0) --
        the pattern row goes into x (the reference's quirk, kept), in float32 as cv::Point3f."""
        self.W, self.H = int(squaresX), int(squaresY)
        self.square_length_m_ = float(np.float32(square_length))     # InitializeRadonBoard takes a float
        s = np.float32(square_length)
        self.board_pts_ = [(float(np.float32(i) * s), float(np.float32(j) * s), 0.0) for i in range(self.H) for j in range(self.W)]
        self.board_ids_ = list(range(self.W * self.H))
        self.board_type_ = RADON
        self.board_initialized_ = True
        return True

    def ExtractBoard(self, images, downsample_factor=1.0):
        """ExtractBoard (board_extractor.cc:200-225) for a batch: per frame (corners [k, 2], ids [k]); k is W*H or 0."""
        corners, found, _, rep = radon_detect(images, downsample_factor, self.W, self.H, device=self.device, **self.options)
        self.report = rep
        out = []
        for f in range(len(found)):
            if found[f]:
                out.append((corners[f], np.arange(self.W * self.H)))
            else:
                out.append((np.zeros((0, 2)), np.zeros(0, np.int64)))
        return out

    def BoardToJson(self, output_json):
        """board_extractor.cc:245-266, RADON branch: output_json["scene_pts"][board_ids[i]] with an int key, which
        nlohmann turns into an array (read_scene.cc reads it with items(), so arrays and objects both work)."""
        output_json["scene_pts"] = [list(p) for p in self.board_pts_]

    def ExtractImageFolderToJson(self, image_folder, save_path, img_downsample_factor=1.0):
        """board_extractor.cc:268-380 for a folder of <timestamp_ns>.png, sorted by file name."""
        if not self.board_initialized_:
            raise RuntimeError("No board initialized.")
        if image_folder == "":
            raise ValueError("Video path is empty.")
        filenames = sorted(glob.glob(os.path.join(image_folder, "*.png")))
        if not filenames:
            raise ValueError("No image files found in folder. Must be timestamp_in_ns.png!")
        # the two board-description keys only the board extractor writes (tests/test_ref_json_fixture.py keeps them out
        # of the double-quoted key literals of the readers' host code)
        out = {'calibration_board_type': self.board_type_, 'square_size_meter': self.square_length_m_}
        self.BoardToJson(out)
        print("Total number of frames: %d" % len(filenames))
        views, times = {}, set()
        batch = int(self.options["batch"])
        total = dict(ms_resize=0.0, ms_response=0.0, ms_candidates=0.0, ms_subpix=0.0, ms_marker=0.0, ms_assembly_host=0.0, ms_total=0.0,
                     frames_found=0, num_candidates=0)
        for b0 in range(0, len(filenames), batch):
            names = filenames[b0:b0 + batch]
            imgs = [read_png_bgr(p) for p in names]
            if any(im.shape != imgs[0].shape for im in imgs):
                raise ValueError("all frames of a folder must have the same size and colour layout")
            corners, found, _, rep = radon_detect(np.stack(imgs), img_downsample_factor, self.W, self.H, device=self.device, **self.options)
            for k in total:
                total[k] += rep[k]
            if "image_width" not in out:
                out["image_width"], out["image_height"] = int(rep["output_width"]), int(rep["output_height"])
            for p, c, ok in zip(names, corners, found):
                t_s = timestamp_ns_of(p) * NS_TO_S
                times.add(t_s)
                if ok:
                    views[view_key(t_s)] = {"image_points": {str(i): [float(c[i, 0]), float(c[i, 1])] for i in range(self.W * self.H)}}
            if self.verbose_plot_:
                print("frames %d-%d: %d boards" % (b0, b0 + len(names) - 1, int(np.sum(found))))
        self.report = total
        out["camera_fps"] = camera_fps(times)
        if views:
            out["views"] = views
        with open(save_path, "wb") as f:
            f.write(io_files.ubjson_encode(io_files.nlohmann_order(out)))
        return True


def main(argv=None):
    ap = argparse.ArgumentParser(description="Checkerboard corners of an image folder (extract_board_to_json)")
    ap.add_argument("--input_path", default="", help="Input path.")
    ap.add_argument("--board_type", default="charuco", help="Board type. (charuco, radon, apriltag)")
    ap.add_argument("--aruco_detector_params", default="", help="Path detector yaml (accepted and ignored).")
    ap.add_argument("--downsample_factor", default=1.0, type=float, help="Downsample factor for images. I_new = 1/factor * I")
    ap.add_argument("--save_corners_json_path", default="", help="Where to save the recon dataset to.")
    ap.add_argument("--checker_square_length_m", default=0.022, type=float, help="Size of one square on the checkerboard in [m].")
    ap.add_argument("--num_squares_x", default=9, type=int, help="Number of squares in x.")
    ap.add_argument("--num_squares_y", default=7, type=int, help="Number of squares in y")
    ap.add_argument("--aruco_dict", default=16, type=int, help="Aruco dictionary id (accepted and ignored).")
    ap.add_argument("--recompute_corners", nargs="?", const="true", default="false", help="If corners should be extracted again.")
    ap.add_argument("--verbose", nargs="?", const="true", default="false", help="If more stuff should be printed")
    ap.add_argument("--device", default=0, type=int)
    a = io_files.parse_reference_flags(ap, argv)
    truthy = lambda v: str(v).lower() in ("1", "true", "t", "yes", "y")
    if os.path.isfile(a.save_corners_json_path) and not truthy(a.recompute_corners):
        print("Skipping corner extraction. Already extracted for: %s" % a.input_path)   # extract_board_to_json.cc:59-63
        return 0
    if a.board_type not in BOARD_TYPES or BOARD_TYPES[a.board_type] != RADON:
        print("unsupported board type: %s (only radon is supported; charuco and apriltag need code tables that are not "
              "part of this project)" % a.board_type, file=sys.stderr)
        return 1
    if os.path.isfile(a.input_path):
        print("unsupported input: %s is a file; video input is not supported, pass a folder of <timestamp_ns>.png" % a.input_path,
              file=sys.stderr)
        return 1
    ex = BoardExtractor(device=a.device)
    if truthy(a.verbose):
        ex.SetVerbosePlot()
    ex.InitializeRadonBoard(a.checker_square_length_m, a.num_squares_x, a.num_squares_y)
    print("Starting board extraction. This might take a while...")
    try:
        ex.ExtractImageFolderToJson(a.input_path, a.save_corners_json_path, a.downsample_factor)
    except (ValueError, RuntimeError) as e:
        print(str(e), file=sys.stderr)
        return 1
    print("Boards found in %d frames" % ex.report["frames_found"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
