"""numpy restatement of the radon board detector (csrc/board.hip + the grid assembly of its host side): the checker of
oicc_board_radon_detect and the specification of its arithmetic, radius, blur and thresholds ("Board
extraction").

  1 resize_gray     centre-aligned bilinear resize with 11-bit weights, then BGR -> gray with 14-bit weights
  2 response        3x3 binomial blur (integers, x16), line sums along 0/45/90/135 degrees over 2r+1 pixels,
                    response ((max - min) / (16 * 255 * (2r+1)))^2 in float32, polarity = index of the brightest line
  3 candidates      threshold rel * frame maximum, strict (2r+1)^2 non-maximum suppression with raster tie-break
  4 subpix          cornerSubPix's gradient-orthogonality iteration on the blurred image (20 iterations, eps 0.01)
  5 assemble        seed quad, homography growth, polarity alternation, W x H
  6 marker / ids    disc vs ring of every square through its homography, three dots, ids i*W + j
"""
import numpy as np

DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1))          # (dx, dy) of the 0, 45, 90 and 135 degree lines
DEFAULTS = dict(radius=3, threshold_rel=0.5, max_candidates=512, subpix_iterations=20, subpix_eps=0.01)


def origin(W, H):
    return (H - 1) // 2, W // 2 - 1


# ---- 1 resize + gray ------------------------------------------------------------------------------------------------
def resize_axis(n_src, factor):
    """Output size and (index, weight of index + 1 in 1/2048) per output sample: sx = (x + 0.5) * scale - 0.5 with
    scale = 1 / (1 / factor) (cv::resize with fx = 1 / factor), clamped at both ends as INTER_LINEAR does."""
    f = 1.0 / float(factor)
    scale = 1.0 / f
    n_dst = int(np.rint(n_src * f))
    idx = np.zeros(n_dst, np.int32)
    w1 = np.zeros(n_dst, np.int32)
    for x in range(n_dst):
        sx = (x + 0.5) * scale - 0.5
        s0 = int(np.floor(sx))
        fx = sx - s0
        if s0 < 0:
            s0, fx = 0, 0.0
        if s0 >= n_src - 1:
            s0, fx = n_src - 1, 0.0
        idx[x] = s0
        w1[x] = int(np.floor(fx * 2048.0 + 0.5))
    return n_dst, idx, w1


def resize_gray(frames, factor):
    """frames [F, h, w] (gray) or [F, h, w, 3] (BGR) u8 -> [F, h', w'] u8."""
    frames = np.asarray(frames, np.uint8)
    F, h, w = frames.shape[:3]
    wd, xi, xw = resize_axis(w, factor)
    hd, yi, yw = resize_axis(h, factor)
    x1 = np.minimum(xi + 1, w - 1); y1 = np.minimum(yi + 1, h - 1)
    src = frames.astype(np.int64)
    if src.ndim == 3:
        src = src[..., None]
    wx0, wx1 = (2048 - xw)[None, None, :, None], xw[None, None, :, None]
    wy0, wy1 = (2048 - yw)[None, :, None, None], yw[None, :, None, None]
    top = src[:, yi][:, :, xi] * wx0 + src[:, yi][:, :, x1] * wx1
    bot = src[:, y1][:, :, xi] * wx0 + src[:, y1][:, :, x1] * wx1
    rs = (top * wy0 + bot * wy1 + (1 << 21)) >> 22
    if rs.shape[-1] == 1:
        return rs[..., 0].astype(np.uint8)
    return ((1868 * rs[..., 0] + 9617 * rs[..., 1] + 4899 * rs[..., 2] + 8192) >> 14).astype(np.uint8)


# ---- 2 response -----------------------------------------------------------------------------------------------------
def blur16(gray):
    """[F, h, w] u8 -> 16 x the 3x3 binomial blur (int32), border replicated."""
    g = np.asarray(gray).astype(np.int32)
    p = np.pad(g, ((0, 0), (0, 0), (1, 1)), mode="edge")
    hz = p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:]
    p = np.pad(hz, ((0, 0), (1, 1), (0, 0)), mode="edge")
    return p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]


def response(B, r):
    """Line sums of the blurred image B (x16 ints) -> response float32 [F,h,w] and polarity u8 (0 within r of the
    border)."""
    F, h, w = B.shape
    sums = []
    for dx, dy in DIRS:
        s = np.zeros((F, h - 2 * r, w - 2 * r), np.int64)
        for k in range(-r, r + 1):
            s += B[:, r + k * dy:h - r + k * dy, r + k * dx:w - r + k * dx]
        sums.append(s)
    S = np.stack(sums)
    inv = np.float32(1.0 / (16.0 * 255.0 * (2 * r + 1)))
    d = (S.max(0) - S.min(0)).astype(np.float32) * inv
    resp = np.zeros((F, h, w), np.float32)
    pol = np.zeros((F, h, w), np.uint8)
    resp[:, r:h - r, r:w - r] = d * d
    pol[:, r:h - r, r:w - r] = S.argmax(0)
    return resp, pol


# ---- 3 candidates ---------------------------------------------------------------------------------------------------
def candidates(resp, r, threshold_rel, max_candidates):
    """Per frame: the (y, x) of strict local maxima in the (2r+1)^2 window (a tie goes to the smaller raster index)
    above threshold_rel * frame maximum, in raster order, and whether the frame overflowed max_candidates."""
    out = []
    F, h, w = resp.shape
    for f in range(F):
        R = resp[f]
        thr = np.float32(threshold_rel) * R.max()
        P = np.pad(R, r, constant_values=-1.0)
        keep = R > thr
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    continue
                N = P[r + dy:r + dy + h, r + dx:r + dx + w]
                later = (dy > 0) or (dy == 0 and dx > 0)          # neighbour has the larger raster index
                keep &= (R > N) | ((R == N) & later)
        ys, xs = np.nonzero(keep)
        out.append((np.stack([ys, xs], 1), len(ys) > max_candidates))
    return out


# ---- 4 sub-pixel refinement -----------------------------------------------------------------------------------------
def _sample(I, x, y, dtype=np.float64):
    h, w = I.shape
    x0 = np.floor(x); y0 = np.floor(y)
    ax = x - x0; ay = y - y0
    xi0 = np.clip(x0.astype(np.int64), 0, w - 1); xi1 = np.clip(x0.astype(np.int64) + 1, 0, w - 1)
    yi0 = np.clip(y0.astype(np.int64), 0, h - 1); yi1 = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    I = I.astype(dtype)
    return (1 - ay) * ((1 - ax) * I[yi0, xi0] + ax * I[yi0, xi1]) + ay * ((1 - ax) * I[yi1, xi0] + ax * I[yi1, xi1])


def subpix(I, xy, win, iterations=20, eps=0.01, dtype=np.float64, trace=None):
    """cornerSubPix (OpenCV imgproc/cornersubpix.cpp) on the float image I for start points xy [n,2]: Gaussian window
    weights exp(-(u/win)^2 - (v/win)^2), central differences of bilinear samples, 2x2 solve per step; stops at
    iterations or a squared step <= eps^2, leaves the image -> stop; a result farther than win from the start -> start.
    dtype: the type of the window, the weights and every sum (np.longdouble runs the same statements in extended
    precision).  trace: a list that receives, per start point, the iterates before the final "farther than win" rule."""
    h, w = I.shape
    u = np.arange(-win, win + 1, dtype=dtype)
    V, U = np.meshgrid(u, u, indexing="ij")
    m = np.exp(-(U / win) ** 2) * np.exp(-(V / win) ** 2)
    out = np.array(xy, dtype)
    for n in range(len(out)):
        c0 = out[n].copy(); c = c0.copy()
        steps = []
        for _ in range(iterations):
            X = c[0] + U; Y = c[1] + V
            gx = _sample(I, X + 1, Y, dtype) - _sample(I, X - 1, Y, dtype)
            gy = _sample(I, X, Y + 1, dtype) - _sample(I, X, Y - 1, dtype)
            gxx, gxy, gyy = gx * gx * m, gx * gy * m, gy * gy * m
            a, b, cc = gxx.sum(), gxy.sum(), gyy.sum()
            bb1 = (gxx * U + gxy * V).sum(); bb2 = (gxy * U + gyy * V).sum()
            det = a * cc - b * b
            if abs(det) <= np.finfo(np.float64).eps ** 2:
                break
            s = 1.0 / det
            c2 = np.array([c[0] + cc * s * bb1 - b * s * bb2, c[1] - b * s * bb1 + a * s * bb2], dtype)
            err = ((c2 - c) ** 2).sum()
            c = c2
            steps.append(c.copy())
            if c[0] < 0 or c[0] >= w or c[1] < 0 or c[1] >= h or err <= eps * eps:
                break
        if abs(c[0] - c0[0]) > win or abs(c[1] - c0[1]) > win:
            c = c0
        out[n] = c
        if trace is not None:
            trace.append(steps)
    return out


# ---- 5 grid assembly ------------------------------------------------------------------------------------------------
def _homography(src, dst):
    """DLT with h33 = 1 on (centred) points; src, dst [n,2], n >= 4."""
    ms, md = src.mean(0), dst.mean(0)
    ss = max(np.abs(src - ms).max(), 1e-12); sd = max(np.abs(dst - md).max(), 1e-12)
    a = (src - ms) / ss; b = (dst - md) / sd
    A = np.zeros((2 * len(a), 8)); y = np.zeros(2 * len(a))
    for k, ((x, yy), (u, v)) in enumerate(zip(a, b)):
        A[2 * k] = [x, yy, 1, 0, 0, 0, -u * x, -u * yy]; y[2 * k] = u
        A[2 * k + 1] = [0, 0, 0, x, yy, 1, -v * x, -v * yy]; y[2 * k + 1] = v
    h = np.linalg.solve(A.T @ A + 1e-12 * np.eye(8), A.T @ y)
    Hn = np.append(h, 1.0).reshape(3, 3)
    T1 = np.array([[1 / ss, 0, -ms[0] / ss], [0, 1 / ss, -ms[1] / ss], [0, 0, 1]])
    T2 = np.array([[sd, 0, md[0]], [0, sd, md[1]], [0, 0, 1]])
    return T2 @ Hn @ T1


def _apply(Hm, p):
    q = Hm @ np.array([p[0], p[1], 1.0])
    return q[:2] / q[2]


def _pol_sign(direction, u, v):
    """+1 when the brightest line (DIRS index) runs between +-u and +-v (same-sign combination), else -1."""
    d = np.array(DIRS[direction], np.float64)
    det = u[0] * v[1] - u[1] * v[0]
    if abs(det) < 1e-12:
        return 0
    al = (d[0] * v[1] - d[1] * v[0]) / det
    be = (u[0] * d[1] - u[1] * d[0]) / det
    return 1 if al * be > 0 else -1


def assemble(pts, pol, resp, W, H, max_seeds=8):
    """Refined candidates pts [n,2] (x, y) with polarity and response -> grid [A, B, 2] of candidate indices with
    {A, B} = {W, H}, or None.  Duplicates (within 1 px) keep the stronger response."""
    order = np.argsort(-resp, kind="stable")
    kept = []
    for i in order:
        if all(np.hypot(*(pts[i] - pts[j])) >= 1.0 for j in kept):
            kept.append(i)
    kept = np.array(kept, np.int64)
    if len(kept) < W * H:
        return None
    P = pts[kept]
    D = np.hypot(P[:, None, 0] - P[None, :, 0], P[:, None, 1] - P[None, :, 1])
    np.fill_diagonal(D, np.inf)
    lim = max(W, H)
    for s0 in range(min(max_seeds, len(P))):
        nn = np.argsort(D[s0], kind="stable")
        c1 = nn[0]; u = P[c1] - P[s0]; du = np.hypot(*u)
        c2 = -1
        for j in nn[1:]:
            v = P[j] - P[s0]; dv = np.hypot(*v)
            if dv > 2.0 * du:
                break
            if abs(u @ v) < 0.6 * du * dv:
                c2 = j; break
        if c2 < 0:
            continue
        v = P[c2] - P[s0]
        pred = P[s0] + u + v
        d3 = np.hypot(P[:, 0] - pred[0], P[:, 1] - pred[1])
        c3 = int(np.argmin(d3))
        if d3[c3] > 0.3 * min(du, np.hypot(*v)) or c3 in (s0, c1, c2):
            continue
        sg = [_pol_sign(pol[kept[c]], u, v) for c in (s0, c1, c2, c3)]
        if not (sg[0] == sg[3] != 0 and sg[1] == sg[2] == -sg[0]):
            continue
        grid = {(0, 0): s0, (1, 0): c1, (0, 1): c2, (1, 1): c3}
        used = set(grid.values())
        ok = True
        while ok:
            changed = False
            amin = min(a for a, _ in grid); amax = max(a for a, _ in grid)
            bmin = min(b for _, b in grid); bmax = max(b for _, b in grid)
            if amax - amin + 1 > lim or bmax - bmin + 1 > lim:
                ok = False; break
            front = sorted({(a + da, b + db) for (a, b) in grid for da, db in ((1, 0), (-1, 0), (0, 1), (0, -1))} - set(grid))
            for (a, b) in front:
                nb = [(x, y) for (x, y) in grid if abs(x - a) <= 2 and abs(y - b) <= 2]
                if len(nb) < 4 or len({x for x, _ in nb}) < 2 or len({y for _, y in nb}) < 2:
                    continue
                Hm = _homography(np.array(nb, np.float64), P[[grid[q] for q in nb]])
                pr = _apply(Hm, (a, b))
                sl = min(np.hypot(*(_apply(Hm, (a + 1, b)) - pr)), np.hypot(*(_apply(Hm, (a, b + 1)) - pr)))
                dd = np.hypot(P[:, 0] - pr[0], P[:, 1] - pr[1])
                j = int(np.argmin(dd))
                if dd[j] < 0.3 * sl and j not in used:
                    grid[(a, b)] = j; used.add(j); changed = True
            if not changed:
                break
        if not ok:
            continue
        amin = min(a for a, _ in grid); amax = max(a for a, _ in grid)
        bmin = min(b for _, b in grid); bmax = max(b for _, b in grid)
        A, B = amax - amin + 1, bmax - bmin + 1
        if sorted((A, B)) != sorted((W, H)) or len(grid) != A * B:
            continue
        G = np.zeros((A, B), np.int64)
        for (a, b), j in grid.items():
            G[a - amin, b - bmin] = j
        if not polarity_alternates(P, pol[kept], G):
            continue
        return kept[G]
    return None


def polarity_alternates(P, pol, G):
    A, B = G.shape
    ref = None
    for a in range(A):
        for b in range(B):
            u = P[G[min(a + 1, A - 1), b]] - P[G[max(a - 1, 0), b]]
            v = P[G[a, min(b + 1, B - 1)]] - P[G[a, max(b - 1, 0)]]
            s = _pol_sign(pol[G[a, b]], u, v) * (1 if (a + b) % 2 == 0 else -1)
            if s == 0 or (ref is not None and s != ref):
                return False
            ref = s
    return True


# ---- 6 marker and ids -----------------------------------------------------------------------------------------------
DISC = [(0.0, 0.0)] + [(0.07 * np.cos(t), 0.07 * np.sin(t)) for t in np.arange(4) * np.pi / 2]
RING = [(0.32 * np.cos(t), 0.32 * np.sin(t)) for t in np.arange(8) * np.pi / 4]


def square_to_quad(q):
    """Homography coefficients (a..h) of the unit square (0,0),(1,0),(1,1),(0,1) -> quad q [4,2] (Heckbert)."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = q
    sx = x0 - x1 + x2 - x3; sy = y0 - y1 + y2 - y3
    dx1 = x1 - x2; dx2 = x3 - x2; dy1 = y1 - y2; dy2 = y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    hh = (dx1 * sy - sx * dy1) / den
    return (x1 - x0 + g * x1, x3 - x0 + hh * x3, x0, y1 - y0 + g * y1, y3 - y0 + hh * y3, y0, g, hh)


def cell_means(I, C, dtype=np.float64):
    """C [A, B, 2] grid corner pixels -> disc and ring means [A-1, B-1] of every square (bilinear samples), computed
    in dtype."""
    C = np.asarray(C, dtype)
    A, B = C.shape[:2]
    disc = np.zeros((A - 1, B - 1), dtype); ring = np.zeros((A - 1, B - 1), dtype)
    for a in range(A - 1):
        for b in range(B - 1):
            k = square_to_quad([C[a, b], C[a + 1, b], C[a + 1, b + 1], C[a, b + 1]])
            for out, pts in ((disc, DISC), (ring, RING)):
                acc = 0.0
                for du, dv in pts:
                    s, t = 0.5 + du, 0.5 + dv
                    den = k[6] * s + k[7] * t + 1.0
                    acc += _sample(I, np.array((k[0] * s + k[1] * t + k[2]) / den), np.array((k[3] * s + k[4] * t + k[5]) / den), dtype)
                out[a, b] = acc / len(pts)
    return disc, ring


def marker_ids(disc, ring, C):
    """Squares' disc/ring means and the grid's corner pixels C [A, B, 2] -> (row axis, column axis, origin) in grid-index space, or None.  The black dot: the
    only white square whose disc is darker than its ring by more than half the contrast; the white dots: the only two
    black squares brighter by as much, 4-neighbours of it and perpendicular."""
    mid = 0.5 * (ring.max() + ring.min())
    white = ring > mid
    contrast = ring[white].mean() - ring[~white].mean() if white.any() and (~white).any() else 0.0
    if contrast <= 0:
        return None
    score = (ring - disc) / contrast
    bl = np.argwhere(white & (score > 0.5))
    wh = np.argwhere(~white & (score < -0.5))
    if len(bl) != 1 or len(wh) != 2:
        return None
    bc = bl[0]
    d = [w - bc for w in wh]
    if any(abs(x).sum() != 1 for x in d) or abs(d[0] @ d[1]) != 0:
        return None
    # which dot is "up" (row - 1) and which "right" (column + 1): a board seen from its printed side has
    # det[right, down] > 0 in the image (columns run right and rows down on the target)
    cen = lambda c: C[c[0]:c[0] + 2, c[1]:c[1] + 2].reshape(4, 2).mean(0)
    pb = cen(bc)
    for up, right in ((d[0], d[1]), (d[1], d[0])):
        ri = cen(bc + right) - pb; dn = pb - cen(bc + up)
        if ri[0] * dn[1] - ri[1] * dn[0] > 0:
            break
    else:
        return None
    row, col = -up, right
    return row, col, bc


def ids_from_marker(grid_shape, row, col, bc, W, H):
    """grid index (a, b) -> id i*W + j (or None if the orientation does not give a W x H board)."""
    A, B = grid_shape
    r0, c0 = origin(W, H)
    cells = [bc + np.array(o) for o in ((0, 0), (1, 0), (0, 1), (1, 1))]
    o = min(cells, key=lambda p: (row @ p, col @ p))
    ids = np.zeros((A, B), np.int64)
    for a in range(A):
        for b in range(B):
            q = np.array([a, b]) - o
            i, j = r0 + row @ q, c0 + col @ q
            if not (0 <= i < H and 0 <= j < W):
                return None
            ids[a, b] = i * W + j
    return ids


# ---- the whole detector ---------------------------------------------------------------------------------------------
def detect(frames, factor, W, H, radius=3, threshold_rel=0.5, max_candidates=512, subpix_iterations=20, subpix_eps=0.01,
           debug=False):
    """frames -> corners [F, W*H, 2] (NaN where not found), found [F] (and the per-stage pieces with debug: per frame also
    the grid of candidate indices [A, B] or None, its shape or (0, 0), and the disc / ring means of its squares)."""
    gray = resize_gray(frames, factor)
    B = blur16(gray)
    resp, pol = response(B, radius)
    I = B.astype(np.float32) * np.float32(1.0 / 16.0)
    cands = candidates(resp, radius, threshold_rel, max_candidates)
    F = gray.shape[0]
    corners = np.full((F, W * H, 2), np.nan); found = np.zeros(F, bool)
    refined_all = []
    grids = [None] * F; shapes = [(0, 0)] * F; discs = [None] * F; rings = [None] * F
    for f in range(F):
        yx, overflow = cands[f]
        ref = subpix(I[f], yx[:, ::-1].astype(np.float64), radius + 2, subpix_iterations, subpix_eps)
        refined_all.append(ref)
        if overflow or len(ref) < W * H:
            continue
        G = assemble(ref, pol[f][yx[:, 0], yx[:, 1]], resp[f][yx[:, 0], yx[:, 1]], W, H)
        if G is None:
            continue
        disc, ring = cell_means(I[f], ref[G])
        grids[f], shapes[f], discs[f], rings[f] = G, G.shape, disc, ring
        m = marker_ids(disc, ring, ref[G])
        if m is None:
            continue
        ids = ids_from_marker(G.shape, *m, W, H)
        if ids is None:
            continue
        corners[f][ids.ravel()] = ref[G.ravel()]
        found[f] = True
    if debug:
        return corners, found, dict(gray=gray, blur=B, response=resp, polarity=pol, candidates=cands, refined=refined_all,
                                    blurred=I, grid=grids, grid_shape=shapes, disc=discs, ring=rings)
    return corners, found
