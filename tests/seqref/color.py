"""Sequential restatement of the input conditioning of Tracking::GrabImageRGBD / GrabImageMonocular
(src/Tracking.cc:167-260): the grey conversion, the depth-map factor and the depth conversion.  Pure Python / numpy,
written per pixel from the stated formulas; imports neither the package under test nor the oracle.

cvtColor itself is OpenCV's: what is restated here is the integer RGB2Gray<uchar> of OpenCV 2.4 - 3.3
    Y = (R*4899 + G*9617 + B*1868 + (1 << 13)) >> 14
generalised to a weight table and shift (a stated, unpinned choice), with the saturation that
weights summing above 1 << shift need.
"""
import numpy as np

GRAY_WEIGHTS = (4899, 9617, 1868)   # wR, wG, wB
GRAY_SHIFT = 14


def cvt_gray(img, rgb, weights=GRAY_WEIGHTS, shift=GRAY_SHIFT):
    """img: uint8 [rows, cols, 3|4]; rgb: byte 0 of a pixel is R (Camera.RGB: 1, src/Tracking.cc:174-177 picks
    CV_RGB2GRAY / CV_RGBA2GRAY), else B (CV_BGR2GRAY / CV_BGRA2GRAY, :178-183).  A fourth channel is ignored."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4)
    wr, wg, wb = (int(w) for w in weights)
    half = 1 << (shift - 1)
    rows, cols = img.shape[:2]
    out = np.zeros((rows, cols), np.uint8)
    for y in range(rows):
        line = img[y].tolist()
        dst = []
        for px in line:
            r, g, b = (px[0], px[1], px[2]) if rgb else (px[2], px[1], px[0])
            v = (r * wr + g * wg + b * wb + half) >> shift
            dst.append(255 if v > 255 else v)
        out[y] = dst
    return out


def depth_map_factor(value):
    """mDepthMapFactor after the Tracking constructor (src/Tracking.cc:142-146): the setting is stored into a float;
    |f| < 1e-5 -> 1, else 1.0f / f (float division)."""
    f = np.float32(value)
    if abs(float(f)) < 1e-5:
        return np.float32(1.0)
    return np.float32(np.float32(1.0) / f)


def depth_to_float(depth, factor):
    """src/Tracking.cc:227-228: if (fabs(mDepthMapFactor - 1.0f) > 1e-5 || imDepth.type() != CV_32F)
    imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor): per pixel one float32 product (an integer sample is exact in
    float32); otherwise the float image is left as it is."""
    depth = np.asarray(depth)
    factor = np.float32(factor)
    diff = np.float32(factor - np.float32(1.0))          # float subtraction
    convert = abs(float(diff)) > 1e-5 or depth.dtype != np.float32
    if not convert:
        return depth
    out = np.zeros(depth.shape, np.float32)
    for y in range(depth.shape[0]):
        for x in range(depth.shape[1]):
            out[y, x] = np.float32(np.float32(depth[y, x]) * factor)
    return out


def grab_image_rgbd(img, depth, rgb, factor):
    """(mImGray, imDepth) as Tracking::GrabImageRGBD hands them to the Frame constructor (:207-231): a grey image goes
    through unchanged (channels() == 1 matches neither branch)."""
    img = np.asarray(img)
    gray = img if img.ndim == 2 else cvt_gray(img, rgb)
    return gray, depth_to_float(depth, factor)
