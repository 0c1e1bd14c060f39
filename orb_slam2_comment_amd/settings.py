"""The part of the example harness that feeds the front-end: the settings file (cv::FileStorage YAML subset read by the
Tracking constructor, src/Tracking.cc:51-147), the KITTI sequence layout of Examples/Monocular/mono_kitti.cc:127-157 and
the TUM lists of Examples/RGB-D/rgbd_tum.cc:142-167 / Examples/Monocular/mono_tum.cc:127-160, and the stereo
rectification matrices and list layout of Examples/Stereo/stereo_euroc.cc:63-98, 192-216.
No OpenCV: scalars are parsed from the text, images are decoded by a small PNG (8-bit grey / RGB / RGBA, 16-bit grey) /
PGM reader."""
import os
import struct
import zlib

import numpy as np

MONOCULAR, STEREO, RGBD = 0, 1, 2      # System::eSensor, include/System.h:46-50


def load_settings(path):
    """`key: scalar` entries of an OpenCV YAML settings file (e.g. Examples/Monocular/KITTI00-02.yaml) as a dict of
    int / float / str.  The `%YAML:1.0` directive, comments and `!!opencv-matrix` blocks are skipped."""
    out = {}
    in_block = False
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].rstrip()
            if not line.strip() or line.startswith("%"):
                continue
            if line[0] in " \t":            # continuation of a nested mapping (matrix rows/cols/dt/data)
                continue
            if ":" not in line:
                continue
            key, val = line.split(":", 1)
            key, val = key.strip(), val.strip()
            in_block = val.startswith("!!") or val == ""
            if in_block:
                continue
            try:
                out[key] = int(val)
            except ValueError:
                try:
                    out[key] = float(val)
                except ValueError:
                    out[key] = val.strip('"')
    return out


def extractor_args(settings):
    """(nFeatures, scaleFactor, nLevels, iniThFAST, minThFAST), src/Tracking.cc:112-116."""
    return (int(settings["ORBextractor.nFeatures"]), float(settings["ORBextractor.scaleFactor"]),
            int(settings["ORBextractor.nLevels"]), int(settings["ORBextractor.iniThFAST"]),
            int(settings["ORBextractor.minThFAST"]))


def make_extractors(settings, sensor, device=0):
    """The extractor objects the Tracking constructor creates (src/Tracking.cc:119-125): left always, right for
    stereo, and the 2*nFeatures initialisation extractor for monocular."""
    from .extractor import ORBextractor
    nf, sf, nl, ini, mn = extractor_args(settings)
    ex = {"left": ORBextractor(nf, sf, nl, ini, mn, device=device)}
    if sensor == STEREO:
        ex["right"] = ORBextractor(nf, sf, nl, ini, mn, device=device)
    if sensor == MONOCULAR:
        ex["ini"] = ORBextractor(2 * nf, sf, nl, ini, mn, device=device)
    return ex


def load_kitti_sequence(path_to_sequence, camera="image_0"):
    """LoadImages of Examples/Monocular/mono_kitti.cc:127-157: timestamps from times.txt (empty lines skipped), file
    names <sequence>/image_0/%06d.png.  Returns (filenames, timestamps)."""
    stamps = []
    with open(os.path.join(path_to_sequence, "times.txt")) as f:
        for s in f:
            if s.strip():
                stamps.append(float(s.split()[0]))
    names = [os.path.join(path_to_sequence, camera, "%06d.png" % i) for i in range(len(stamps))]
    return names, stamps


def read_gray_image(path):
    """8-bit grayscale image as a 2-D uint8 array.  Supports non-interlaced 8-bit grayscale PNG (what KITTI odometry
    ships), binary PGM (P5, maxval 255) and .npy."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("%s: expected a 2-D uint8 array" % path)
        return np.ascontiguousarray(a)
    if path.endswith(".png"):
        try:                                        # C decoder when Pillow happens to be installed
            from PIL import Image
            with Image.open(path) as im:
                if im.mode == "L":
                    return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
        except Exception:                           # Pillow absent or unable to read it: the reader below decides
            pass
    return _read_gray_image_py(path)


def _read_gray_image_py(path):
    data = open(path, "rb").read()
    if data[:2] == b"P5":
        parts, pos = [], 2
        while len(parts) < 3:                       # width, height, maxval separated by whitespace / comments
            while data[pos:pos + 1].isspace():
                pos += 1
            if data[pos:pos + 1] == b"#":
                pos = data.index(b"\n", pos) + 1
                continue
            end = pos
            while not data[end:end + 1].isspace():
                end += 1
            parts.append(int(data[pos:end]))
            pos = end
        w, h, maxval = parts
        if maxval != 255:
            raise ValueError("%s: only 8-bit PGM is supported" % path)
        return np.frombuffer(data, np.uint8, w * h, pos + 1).reshape(h, w).copy()
    hdr, rows = _png_rows(path, data)
    w, h, depth, ctype = hdr
    if depth != 8 or ctype != 0:
        raise ValueError("%s: only non-interlaced 8-bit grayscale PNG is supported (depth %d, colour type %d)"
                         % (path, depth, ctype))
    return rows


def _png_rows(path, data):
    """Defiltered scanlines of a non-interlaced PNG with whole-byte samples: ((w, h, depth, colour type), uint8 [h, w*bpp])."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s: not a PNG / PGM / npy file" % path)
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("%s: no IHDR" % path)
    w, h, depth, ctype, _, _, interlace = hdr
    samples = {0: 1, 2: 3, 4: 2, 6: 4}.get(ctype)
    if interlace != 0 or depth not in (8, 16) or samples is None:
        raise ValueError("%s: only non-interlaced PNG with 8- or 16-bit samples is supported (depth %d, colour type %d, "
                         "interlace %d)" % (path, depth, ctype, interlace))
    bpp = samples * depth // 8                       # the filters' "pixel to the left" is bpp bytes back
    nb = w * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, nb + 1)
    out = np.zeros((h, nb), np.uint8)
    prev = np.zeros(nb, np.uint8)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 2:
            cur = line + prev                        # uint8 wrap-around is the PNG arithmetic
        elif ft == 1:                                # Sub: a running sum per byte lane of the pixel
            cur = np.zeros(nb, np.uint8)
            for k in range(bpp):
                cur[k::bpp] = np.cumsum(line[k::bpp], dtype=np.uint64).astype(np.uint8)
        else:                                        # Average / Paeth depend on the pixel to the left: serial in x
            cur = np.zeros(nb, np.uint8)
            up = prev.astype(np.int32)
            ln = line.astype(np.int32)
            for x in range(nb):
                left = int(cur[x - bpp]) if x >= bpp else 0
                if ft == 3:
                    pred = (left + int(up[x])) >> 1
                else:
                    ul = int(up[x - bpp]) if x >= bpp else 0
                    p = left + int(up[x]) - ul
                    pa, pb, pc = abs(p - left), abs(p - int(up[x])), abs(p - ul)
                    pred = left if (pa <= pb and pa <= pc) else (int(up[x]) if pb <= pc else ul)
                cur[x] = (int(ln[x]) + pred) & 255
        out[y] = cur
        prev = cur
    return (w, h, depth, ctype), out


def read_color_image(path):
    """What cv::imread(.., CV_LOAD_IMAGE_UNCHANGED) hands Examples/RGB-D/rgbd_tum.cc:76 and mono_tum.cc:69 for an 8-bit
    image: uint8 [rows, cols, 3|4] in imread's channel order, B first (BGR / BGRA; a PNG stores R first, so bytes 0 and
    2 of every pixel are swapped on the way), for PNG colour types 2 / 6; uint8 [rows, cols] for a grey file.  What the
    bytes mean is then the settings file's business, as in the reference: Camera.RGB (camera_rgb) says whether
    Tracking reads byte 0 as R.  .npy arrays of those shapes are returned as they are (the writer chose the order)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] in (3, 4))):
            raise ValueError("%s: expected a uint8 [rows, cols] or [rows, cols, 3|4] array" % path)
        return np.ascontiguousarray(a)
    data = open(path, "rb").read()
    if data[:2] == b"P5":
        return _read_gray_image_py(path)
    (w, h, depth, ctype), rows = _png_rows(path, data)
    if depth != 8 or ctype not in (0, 2, 6):
        raise ValueError("%s: expected an 8-bit grey, RGB or RGBA PNG (depth %d, colour type %d)" % (path, depth, ctype))
    if ctype == 0:
        return rows
    img = rows.reshape(h, w, 3 if ctype == 2 else 4)
    img[..., [0, 2]] = img[..., [2, 0]]              # R G B [A] in the file -> B G R [A], as imread delivers it
    return img


def read_depth_image(path):
    """The depth image of rgbd_tum.cc:77 as stored: uint16 [rows, cols] from a 16-bit grey PNG (big-endian samples) or a
    uint16 / float32 .npy.  Scaling is left to ComputeStereoFromRGBDRaw (src/Tracking.cc:227-228)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.dtype not in (np.uint16, np.float32):
            raise ValueError("%s: expected a 2-D uint16 or float32 array" % path)
        return np.ascontiguousarray(a)
    (w, h, depth, ctype), rows = _png_rows(path, open(path, "rb").read())
    if depth != 16 or ctype != 0:
        raise ValueError("%s: expected a 16-bit grey PNG (depth %d, colour type %d)" % (path, depth, ctype))
    return rows.view(">u2").astype(np.uint16)


def camera_rgb(settings):
    """mbRGB (src/Tracking.cc:103-104): Camera.RGB != 0, absent = 0 (BGR)."""
    return bool(int(settings.get("Camera.RGB", 0)))


def depth_map_factor(settings):
    """mDepthMapFactor as the Tracking constructor leaves it (src/Tracking.cc:140-147), a float32: 1 / DepthMapFactor, or 1
    when |DepthMapFactor| < 1e-5.  Only stereo / RGB-D sensors read the key; absent = 1."""
    if "DepthMapFactor" not in settings:
        return np.float32(1.0)
    f = np.float32(settings["DepthMapFactor"])
    if abs(float(f)) < 1e-5:
        return np.float32(1.0)
    return np.float32(1.0) / f


def th_depth(settings):
    """mThDepth as the Tracking constructor evaluates it for a stereo / RGB-D sensor (src/Tracking.cc:134-138), a float32:
    mbf * (float)ThDepth / fx with mbf = Camera.bf and fx = Camera.fx read as floats, the product first.  A monocular
    settings file has neither Camera.bf nor ThDepth: KeyError."""
    mbf, fx = np.float32(settings["Camera.bf"]), np.float32(settings["Camera.fx"])
    return np.float32(np.float32(mbf * np.float32(settings["ThDepth"])) / fx)


def load_tum_association(path):
    """LoadImages of Examples/RGB-D/rgbd_tum.cc:142-167: lines `t rgb_file t depth_file`, empty lines skipped.
    Returns (rgb filenames, depth filenames, timestamps)."""
    rgb, dep, stamps = [], [], []
    with open(path) as f:
        for s in f:
            s = s.rstrip("\n")
            if not s:
                continue
            p = s.split()
            stamps.append(float(p[0])); rgb.append(p[1]); dep.append(p[3])
    return rgb, dep, stamps


def load_tum_rgb_list(path):
    """LoadImages of Examples/Monocular/mono_tum.cc:127-160: three header lines skipped, then `t file`.
    Returns (filenames, timestamps)."""
    names, stamps = [], []
    with open(path) as f:
        lines = f.read().split("\n")[3:]
    for s in lines:
        if not s:
            continue
        p = s.split()
        stamps.append(float(p[0])); names.append(p[1])
    return names, stamps


# ---- stereo rectification settings and the EuRoC list layout (Examples/Stereo/stereo_euroc.cc) -------------------------
def load_matrices(path):
    """Every `key: !!opencv-matrix` block of an OpenCV YAML file as a dict of float64 [rows, cols] arrays.  `rows`, `cols`,
    `dt` (d or f) and `data: [...]`, which may run over several lines and may be written `data:[` without a space
    (Examples/Stereo/EuRoC.yaml:43)."""
    out = {}
    key, fields, data = None, {}, None

    def close():
        if key is None:
            return
        if data is None or "rows" not in fields or "cols" not in fields:
            raise ValueError("%s: matrix %s is incomplete" % (path, key))
        vals = [float(v) for v in data.replace("[", " ").replace("]", " ").split(",") if v.strip()]
        r, c = int(fields["rows"]), int(fields["cols"])
        if len(vals) != r * c:
            raise ValueError("%s: matrix %s has %d values for %dx%d" % (path, key, len(vals), r, c))
        if fields.get("dt", "d") not in ("d", "f"):
            raise ValueError("%s: matrix %s: unsupported dt %r" % (path, key, fields.get("dt")))
        out[key] = np.array(vals, np.float64).reshape(r, c)

    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].rstrip()
            if not line.strip() or line.startswith("%"):
                continue
            if line[0] not in " \t":                     # a top-level key ends the block before it
                close()
                key, fields, data = None, {}, None
                k, _, v = line.partition(":")
                if v.strip().startswith("!!opencv-matrix"):
                    key = k.strip()
                continue
            if key is None:
                continue
            body = line.strip()
            if data is not None and "]" not in data:      # continuation of a data list
                data += " " + body
                continue
            k, _, v = body.partition(":")
            if k.strip() == "data":
                data = v.strip()
            else:
                fields[k.strip()] = v.strip().strip('"')
    close()
    return out


def stereo_rectification(path):
    """What stereo_euroc.cc:63-94 reads: {"left" | "right": {"K", "D", "R", "P", "width", "height"}}, K / R 3x3, P 3x4, D a
    flat coefficient vector.  Raises ValueError with the example's message when a matrix is empty or a size is 0."""
    st, mats = load_settings(path), load_matrices(path)
    out = {}
    for side, pre in (("left", "LEFT."), ("right", "RIGHT.")):
        cam = {k: mats.get(pre + k) for k in "KDRP"}
        cam["height"], cam["width"] = int(st.get(pre + "height", 0)), int(st.get(pre + "width", 0))
        if any(cam[k] is None or cam[k].size == 0 for k in "KDRP") or cam["height"] == 0 or cam["width"] == 0:
            raise ValueError("ERROR: Calibration parameters to rectify stereo are missing!")
        cam["D"] = cam["D"].reshape(-1)
        out[side] = cam
    return out


def load_euroc_sequence(left_dir, right_dir, times_file):
    """LoadImages of Examples/Stereo/stereo_euroc.cc:192-216: one stamp per non-empty line of the times file, images
    <dir>/<line>.png, time = line / 1e9.  Returns (left names, right names, timestamps)."""
    left, right, stamps = [], [], []
    with open(times_file) as f:
        for s in f:
            s = s.strip()
            if s:
                left.append(left_dir + "/" + s + ".png")
                right.append(right_dir + "/" + s + ".png")
                stamps.append(float(s) / 1e9)
    return left, right, stamps
