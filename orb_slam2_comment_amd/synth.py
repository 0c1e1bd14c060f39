"""Deterministic synthetic camera frames.

No KITTI/EuRoC data exists in this environment, so every benchmark and parity
test uses `synth_frame(seed, W, H)`: a smooth random background, filled
rectangles and discs (corner-rich, KITTI-like FAST candidate density) and +-3
uniform noise.  `synth_stereo` renders the same layered scene from a second
eye with a per-shape horizontal disparity, so uL - uR = d for every shape.
"""
import numpy as np


def _scene(seed, W, H, n_rect, n_disc, n_small=None):
    rng = np.random.default_rng(seed)
    if n_small is None:  # fine texture (foliage/gravel stand-in), scaled with the area
        n_small = int(3000 * (W * H) / (1241.0 * 376.0))
    gy, gx = 9, 17
    grid = rng.uniform(40, 215, size=(gy, gx))
    shapes = []
    for _ in range(n_rect):
        w, h = rng.integers(8, 121, size=2)
        x0 = rng.integers(-w // 2, W - w // 2)
        y0 = rng.integers(-h // 2, H - h // 2)
        shapes.append(("r", int(x0), int(y0), int(w), int(h), int(rng.integers(0, 256)),
                       int(rng.integers(2, 81))))
    for _ in range(n_disc):
        r = rng.integers(3, 31)
        cx = rng.integers(0, W)
        cy = rng.integers(0, H)
        shapes.append(("d", int(cx), int(cy), int(r), 0, int(rng.integers(0, 256)),
                       int(rng.integers(2, 81))))
    for _ in range(n_small):
        w, h = rng.integers(2, 11, size=2)
        x0 = rng.integers(0, W)
        y0 = rng.integers(0, H)
        shapes.append(("r", int(x0), int(y0), int(w), int(h), int(rng.integers(0, 256)),
                       int(rng.integers(2, 81))))
    # paint far-to-near so that larger disparity (nearer) occludes
    shapes.sort(key=lambda s: s[6])
    return grid, shapes


def _background(grid, W, H):
    gy, gx = grid.shape
    ys = np.linspace(0, gy - 1, H)
    xs = np.linspace(0, gx - 1, W)
    y0 = np.clip(np.floor(ys).astype(int), 0, gy - 2)
    x0 = np.clip(np.floor(xs).astype(int), 0, gx - 2)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    g = grid
    return ((1 - fy) * (1 - fx) * g[y0][:, x0] + (1 - fy) * fx * g[y0][:, x0 + 1]
            + fy * (1 - fx) * g[y0 + 1][:, x0] + fy * fx * g[y0 + 1][:, x0 + 1])


def _render(grid, shapes, W, H, eye_shift, noise_seed, shift_xy=(0, 0)):
    img = _background(grid, W, H)
    sx, sy = shift_xy
    for kind, a, b, c, d, gray, disp in shapes:
        off = -disp if eye_shift else 0
        if kind == "r":
            x0, y0, w, h = a + off + sx, b + sy, c, d
            xa, xb = max(x0, 0), min(x0 + w, W)
            ya, yb = max(y0, 0), min(y0 + h, H)
            if xa < xb and ya < yb:
                img[ya:yb, xa:xb] = gray
        else:
            cx, cy, r = a + off + sx, b + sy, c
            xa, xb = max(cx - r, 0), min(cx + r + 1, W)
            ya, yb = max(cy - r, 0), min(cy + r + 1, H)
            if xa < xb and ya < yb:
                yy, xx = np.ogrid[ya:yb, xa:xb]
                m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
                img[ya:yb, xa:xb][m] = gray
    rng = np.random.default_rng(noise_seed)
    img = img + rng.integers(-3, 4, size=(H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def synth_frame(seed, W=1241, H=376, n_rect=400, n_disc=200, shift_xy=(0, 0)):
    """uint8 [H, W] frame; `shift_xy` translates the shapes (frame t -> t+1)."""
    grid, shapes = _scene(seed, W, H, n_rect, n_disc)
    return _render(grid, shapes, W, H, False, (seed << 8) + 1 + 7 * shift_xy[0] + 13 * shift_xy[1],
                   shift_xy)


def synth_stereo(seed, W=1241, H=376, n_rect=400, n_disc=200, shift_xy=(0, 0)):
    """(left, right) uint8 frames of one layered scene; disparities in [2, 80] px.  `shift_xy` translates the shapes in
    both eyes (stereo frame t -> t+1)."""
    grid, shapes = _scene(seed, W, H, n_rect, n_disc)
    ns = 7 * shift_xy[0] + 13 * shift_xy[1]
    left = _render(grid, shapes, W, H, False, (seed << 8) + 1 + ns, shift_xy)
    right = _render(grid, shapes, W, H, True, (seed << 8) + 2 + ns, shift_xy)
    return left, right


def synth_batch(first_seed, count, W=1241, H=376):
    """uint8 [count, H, W]"""
    return np.stack([synth_frame(first_seed + i, W, H) for i in range(count)])


def synth_color_frame(seed, W=1241, H=376, channels=3, rgb=True):
    """uint8 [H, W, channels] colour frame: three differently seeded renders of one scene as R, G, B (so the channels
    differ), stored R first when `rgb` else B first; with channels == 4 the alpha plane is uniform noise, so that a
    conversion which reads it shows."""
    assert channels in (3, 4)
    grid, shapes = _scene(seed, W, H, 400, 200)
    planes = []
    for c in range(3):
        rng = np.random.default_rng((seed << 8) + 64 + c)
        tint = [(k, a, b, cc, d, int(rng.integers(0, 256)), disp) for k, a, b, cc, d, _, disp in shapes]
        planes.append(_render(grid + rng.uniform(-30, 30, grid.shape), tint, W, H, False, (seed << 8) + 80 + c))
    if not rgb:
        planes.reverse()
    if channels == 4:
        planes.append(np.random.default_rng((seed << 8) + 99).integers(0, 256, (H, W), dtype=np.uint8))
    return np.ascontiguousarray(np.stack(planes, axis=2))


def synth_depth(seed, W=640, H=480):
    """uint16 [H, W] raw depth image in the manner of a TUM RGB-D frame (5000 units per metre): smooth ramps between
    0.5 m and 8 m, about 10 % zero holes (no reading) in blocks, and a few saturated 65535 pixels."""
    rng = np.random.default_rng((seed << 8) + 7)
    grid = rng.uniform(2500, 40000, size=(5, 7))
    d = np.rint(_background(grid, W, H)).astype(np.uint16)
    holes = rng.uniform(size=((H + 7) // 8, (W + 7) // 8)) < 0.10
    d[np.kron(holes, np.ones((8, 8), bool))[:H, :W]] = 0
    ys, xs = rng.integers(0, H, 24), rng.integers(0, W, 24)
    d[ys, xs] = 65535
    return d


def unrectify(img, K, D, R, P, size=None):
    """The raw camera frame whose rectification (initUndistortRectifyMap + remap with the same K, D, R, P) shows `img`:
    every raw pixel is normalised with K, undistorted by the usual 5-step fixed point, rotated by R, projected by P and
    `img` is sampled there bilinearly (edge pixels repeated).  Test / benchmark input only: nothing is compared with it.
    size = (cols, rows) of the raw frame, default img's."""
    K, P = np.asarray(K, np.float64).reshape(3, 3), np.asarray(P, np.float64)[:3, :3]
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    D = list(np.asarray(D, np.float64).reshape(-1)) + [0.0] * 8
    k1, k2, p1, p2, k3 = D[:5]
    cols, rows = (img.shape[1], img.shape[0]) if size is None else size
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    A = P @ R
    w = A[2, 0] * x + A[2, 1] * y + A[2, 2]
    xr = np.clip((A[0, 0] * x + A[0, 1] * y + A[0, 2]) / w, 0, img.shape[1] - 1)
    yr = np.clip((A[1, 0] * x + A[1, 1] * y + A[1, 2]) / w, 0, img.shape[0] - 1)
    xi, yi = np.minimum(xr.astype(np.int64), img.shape[1] - 2), np.minimum(yr.astype(np.int64), img.shape[0] - 2)
    fx, fy = xr - xi, yr - yi
    f = img.astype(np.float64)
    out = (f[yi, xi] * (1 - fx) + f[yi, xi + 1] * fx) * (1 - fy) + (f[yi + 1, xi] * (1 - fx) + f[yi + 1, xi + 1] * fx) * fy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def synth_raw_stereo(seed, calib, W=752, H=480):
    """A raw (unrectified) stereo pair for settings.stereo_rectification's `calib`: synth_stereo seen through the two
    cameras' distortion and rotation.  Returns (raw_left, raw_right)."""
    left, right = synth_stereo(seed, W, H)
    return tuple(unrectify(im, c["K"], c["D"], c["R"], c["P"]) for im, c in ((left, calib["left"]), (right, calib["right"])))


def synth_vocabulary(k=10, L=6, seed=1):
    """Regular k-ary vocabulary tree with the shape of ORBvoc.txt (k=10, L=6: 1.1 M nodes, 10^6 words) in
    saveToTextFile (BFS) order, for benchmarks: the real vocabulary is not part of the reference checkout.
    Children are their parent with a few random bit flips.  Returns (parent, is_leaf, desc, weight), entry i = node i+1,
    ready for ORBVocabulary.from_arrays."""
    rng = np.random.default_rng(seed)
    parent, leaf, desc = [], [], []
    prev_desc, prev_first = rng.integers(0, 256, (1, 32), dtype=np.uint8), 0
    nid = 1
    for depth in range(1, L + 1):
        n = prev_desc.shape[0] * k
        d = np.repeat(prev_desc, k, axis=0)
        for _ in range(max(2, 48 >> depth)):
            bit = rng.integers(0, 256, n)
            d[np.arange(n), bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
        parent.append(np.repeat(np.arange(prev_first, prev_first + prev_desc.shape[0], dtype=np.int32), k))
        leaf.append(np.full(n, depth == L, np.uint8))
        desc.append(d)
        prev_desc, prev_first = d, nid
        nid += n
    parent, leaf, desc = np.concatenate(parent), np.concatenate(leaf), np.concatenate(desc)
    weight = np.where(leaf == 1, rng.uniform(0.5, 12.0, len(leaf)), 0.0)
    return parent, leaf, desc, weight
