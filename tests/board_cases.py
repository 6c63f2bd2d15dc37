"""Cases shared by the CPU and GPU tests of the radon board detector at its edges: frames whose sizes sit around the response
kernel's 64 x 16 tile and its word staging, frames with exact ties, frames over the candidate cap, small marker boards, and the
restatement's results for them in float64 and in x87 extended precision.  numpy and synthetic.radon_board_shade only: no renderer
and no GPU.  Everything here is computed once per process (lru_cache) and must be left unchanged by the tests."""
import functools

import numpy as np

import board_restatement as BR
from openimucameracalibrator_amd import synthetic as S

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
RADII = (1, 3, 8)
THRESHOLDS = (0.0, 0.5, 1.0)
# output sizes (h', w') around the 64 x 16 tile: one tile, one pixel more in both, two tiles and a pixel; widths that are whole
# 4-byte words (192, and 68 with a last tile of 4 pixels) and widths with w % 4 = 2, 3, 1
TILE_SIZES = ((16, 64), (17, 65), (33, 129), (48, 192), (20, 68), (31, 130), (20, 67), (50, 197))
RESIZE_FACTORS = (1.0, 2.0, 1.5, 3.0, 1.3, 0.75)          # 2.0: weight 1024, the tie of >> 22; 3.0: zero weights; 0.75: upsampling
RESIZE_SOURCES = ((19, 64), (64, 65), (65, 197), (197, 19))   # (h, w): odd and even output sizes in both axes
CAP_WIDE = 4096                                            # a cap no frame of these sizes reaches (50 * 197 / 4 < 4096 at r = 1)


def sizes_for(r):
    """The smallest legal image (2r + 3 square) and every tile size the radius fits in."""
    n = 2 * r + 3
    return ((n, n),) + tuple(s for s in TILE_SIZES if min(s) >= n)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- frames ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_frames(h, w, channels=1):
    """[3, h, w] (or [3, h, w, 3]) u8 from a fixed seed: two frames of uniform noise and one of only 0 and 255."""
    rng = np.random.RandomState(1000003 * h + 1009 * w + channels)
    shape = (3, h, w) if channels == 1 else (3, h, w, channels)
    f = rng.randint(0, 256, shape).astype(np.uint8)
    f[2] = np.where(f[2] >= 128, 255, 0)
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def checker_frame(h, w):
    """Axis-aligned checker with squares of 12 pixels: the corners lie between pixels, so the response has 2 x 2 plateaus (in-window
    ties for the non-maximum suppression) and pixels whose brightest line is tied between two directions."""
    y, x = np.mgrid[0:h, 0:w]
    return _frozen(np.where(((x + 5) // 12 + (y + 3) // 12) % 2 == 1, 200, 40).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def constant_frame(h, w):
    return _frozen(np.full((h, w), 128, np.uint8))


@functools.lru_cache(maxsize=None)
def edge_frames(h, w):
    """[5, h, w]: the three random frames, the checker and the constant frame."""
    return _frozen(np.concatenate([random_frames(h, w), checker_frame(h, w)[None], constant_frame(h, w)[None]]))


# (W, H, square px, (h, w), radius, rotation deg); at 97 degrees the grid comes out with A and B swapped
SMALL_BOARDS = ((4, 3, 8, (48, 67), 1, 5.0),
                (4, 3, 14, (80, 100), 3, 7.0),
                (4, 3, 14, (80, 100), 2, 97.0),
                (5, 4, 12, (81, 97), 3, 200.0),
                (6, 5, 20, (150, 170), 5, 33.0),
                (4, 3, 30, (130, 193), 8, 12.0))
SHEAR, PERSPECTIVE = 0.05, 3e-4


@functools.lru_cache(maxsize=None)
def small_board(W, H, square, size, rotation_deg):
    """[h, w] u8: synthetic.radon_board_shade seen through an inverse affine map (rotation, shear 0.05) with a perspective
    denominator (3e-4 per pixel), 4 x 4 samples per pixel, grey levels 30 (black) to 220 (white)."""
    h, w = size
    sub = (np.arange(4) + 0.5) / 4.0 - 0.5
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    px = (x[..., None, None] + sub[None, None, None, :]) - (w - 1) / 2.0
    py = (y[..., None, None] + sub[None, None, :, None]) - (h - 1) / 2.0
    q = 1.0 + PERSPECTIVE * px + 0.5 * PERSPECTIVE * py
    qx, qy = px / q, py / q
    qx = qx + SHEAR * qy
    a = np.deg2rad(rotation_deg)
    bx = np.cos(a) * qx + np.sin(a) * qy            # image -> board: the rotation undone
    by = -np.sin(a) * qx + np.cos(a) * qy
    v = bx / square + (W - 1) / 2.0                 # pattern column runs right, pattern row down: the printed side
    u = by / square + (H - 1) / 2.0
    shade = S.radon_board_shade(u, v, W, H).mean(axis=(2, 3))
    return _frozen(np.rint(30.0 + 190.0 * shade).astype(np.uint8))


def board_frame(k):
    W, H, sq, size, r, rot = SMALL_BOARDS[k]
    return small_board(W, H, sq, size, rot)


# ---- the restatement's stages ------------------------------------------------------------------------------------------
def stages(frames, factor, r, threshold_rel):
    """gray, blurred (float32), response, polarity and the candidate lists [(y, x)] of the restatement."""
    gray = BR.resize_gray(frames, factor)
    B = BR.blur16(gray)
    resp, pol = BR.response(B, r)
    cands = [yx for yx, _ in BR.candidates(resp, r, threshold_rel, 1 << 30)]
    return dict(gray=gray, blur16=B, blurred=B.astype(np.float32) * np.float32(1.0 / 16.0), response=resp, polarity=pol, candidates=cands)


@functools.lru_cache(maxsize=None)
def edge_stages(h, w, r, threshold_rel):
    return stages(edge_frames(h, w), 1.0, r, threshold_rel)


def nms_ties(resp, yx, r):
    """How many of the candidates (y, x) have another pixel of exactly their response inside their (2r+1)^2 window."""
    h, w = resp.shape
    n = 0
    for y, x in yx:
        win = resp[max(y - r, 0):min(y + r + 1, h), max(x - r, 0):min(x + r + 1, w)]
        n += int((win == resp[y, x]).sum() > 1)
    return n


def polarity_ties(B, r):
    """How many pixels (per frame of the x16 blur B) have two directions tied for the brightest line."""
    F, h, w = B.shape
    sums = []
    for dx, dy in BR.DIRS:
        s = np.zeros((F, h - 2 * r, w - 2 * r), np.int64)
        for k in range(-r, r + 1):
            s += B[:, r + k * dy:h - r + k * dy, r + k * dx:w - r + k * dx]
        sums.append(s)
    Sm = np.stack(sums)
    return ((Sm == Sm.max(0)).sum(0) > 1).sum(axis=(1, 2))


# ---- sub-pixel steps in float64 and extended precision ----------------------------------------------------------------
MULTIPLE_LIMIT = 256.0        # no comparison constant may exceed this: a measured multiple above 64, times four, is a finding


def subpix_case(I, yx, r, iterations):
    """The restatement's refined points of candidates yx on the float image I after `iterations` steps with eps = 0, in float64 and
    longdouble, and what a comparison needs to know about them:
      yardstick  largest |float64 - longdouble| over the compared candidates, floored at eps64 * max(w, h)
      aside      candidates whose decisions could flip within tol = MULTIPLE_LIMIT * (that difference over all candidates, floored):
                 a move within tol of win (the "moved more than the window" reset), an iterate within tol of the image bounds (the
                 "leaves the image" stop), or a different number of steps in the two precisions
      reset, left, singular   which candidates took the reset, the leaves-the-image stop, the singular-matrix stop (longdouble run)."""
    h, w = I.shape
    win = r + 2
    xy = yx[:, ::-1].astype(np.float64)
    t64, tld = [], []
    r64 = BR.subpix(I, xy, win, iterations, 0.0, trace=t64)
    rld = BR.subpix(I, xy, win, iterations, 0.0, dtype=LD, trace=tld)
    floor = EPS64 * max(w, h)
    n = len(xy)
    same = np.array([len(t64[k]) == len(tld[k]) for k in range(n)], bool)
    diff = np.abs(r64.astype(LD) - rld).max(axis=1).astype(np.float64) if n else np.zeros(0)
    tol = MULTIPLE_LIMIT * max(float(diff[same].max()) if same.any() else 0.0, floor)
    aside = ~same
    reset = np.zeros(n, bool); left = np.zeros(n, bool); singular = np.zeros(n, bool)
    for k in range(n):
        steps = tld[k]
        singular[k] = len(steps) < iterations and not (steps and _outside(steps[-1], w, h))
        for c in steps:
            left[k] |= _outside(c, w, h)
            if min(abs(float(c[0])), abs(float(c[0]) - w), abs(float(c[1])), abs(float(c[1]) - h)) <= tol:
                aside[k] = True
        if steps:
            d = np.abs(np.array(steps[-1], np.float64) - xy[k])
            reset[k] = bool((d > win).any())
            if (np.abs(d - win) <= tol).any():
                aside[k] = True
    keep = ~aside
    yard = max(float(diff[keep].max()) if keep.any() else 0.0, floor)
    return dict(f64=r64, ld=rld, yardstick=yard, floor=floor, tol=tol, aside=aside, reset=reset, left=left, singular=singular)


def _outside(c, w, h):
    return bool(c[0] < 0 or c[0] >= w or c[1] < 0 or c[1] >= h)


SUBPIX_RANDOM = ((1, (17, 65)), (3, (33, 129)), (8, (48, 192)), (1, (50, 197)))       # (radius, (h, w)): random frames, threshold 0
SUBPIX_STEPS = (1, 3)


@functools.lru_cache(maxsize=None)
def subpix_random_case(r, size, iterations):
    """Per frame of random_frames(size) the subpix_case of all candidates at threshold 0."""
    st = stages(random_frames(*size), 1.0, r, 0.0)
    return st, [subpix_case(st["blurred"][f], st["candidates"][f], r, iterations) for f in range(3)]


@functools.lru_cache(maxsize=None)
def subpix_board_case(k, iterations):
    W, H, sq, size, r, rot = SMALL_BOARDS[k]
    st = stages(board_frame(k)[None], 1.0, r, 0.5)
    return st, [subpix_case(st["blurred"][0], st["candidates"][0], r, iterations)]


# ---- whole detector on the small boards ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def board_detection(k):
    """BR.detect(debug=True) of small board k at the default options but its radius."""
    W, H, sq, size, r, rot = SMALL_BOARDS[k]
    return BR.detect(board_frame(k)[None], 1.0, W, H, radius=r, debug=True)


def marker_case(I, C):
    """disc / ring means of grid corners C on the float image I in float64 and longdouble, with the yardsticks (floored at eps64 * 255)."""
    d64, r64 = BR.cell_means(I, C)
    dld, rld = BR.cell_means(I, C, dtype=LD)
    floor = EPS64 * 255.0
    return dict(disc=dld, ring=rld, yard_disc=max(float(np.abs(d64 - dld).max()), floor), yard_ring=max(float(np.abs(r64 - rld).max()), floor))


# ---- overflow -----------------------------------------------------------------------------------------------------------
OVERFLOW_SIZE, OVERFLOW_RADIUS = (50, 197), 1


@functools.lru_cache(maxsize=None)
def overflow_counts():
    """Candidates per random frame of 50 x 197 at r = 1, threshold 0."""
    st = stages(random_frames(*OVERFLOW_SIZE), 1.0, OVERFLOW_RADIUS, 0.0)
    return st, [len(c) for c in st["candidates"]]


MIXED_BOARD, MIXED_BOARD_TURNED = 1, None     # small board 1 (4 x 3, 14 px, 80 x 100, r = 3, 7 degrees) and the same turned by 90


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Five frames of 80 x 100 for one call with batch = 2: constant, the small board, a frame over the cap, the board turned by 90
    degrees, random.  Returns (frames, options, the restatement's detect(debug=True) at these options)."""
    W, H, sq, size, r, rot = SMALL_BOARDS[MIXED_BOARD]
    h, w = size
    frames = np.stack([constant_frame(h, w), small_board(W, H, sq, size, rot), checker_frame(h, w), small_board(W, H, sq, size, rot + 90.0),
                       random_frames(h, w)[0]])
    counts = [len(yx) for yx in stages(frames, 1.0, r, 0.5)["candidates"]]
    cap = max(counts[1], counts[3], counts[4])          # the boards and the random frame fit exactly or with room; the checker does not
    opt = dict(radius=r, threshold_rel=0.5, max_candidates=cap)
    return _frozen(frames), opt, counts, BR.detect(frames, 1.0, W, H, debug=True, **opt)
