"""The calls that the image operators of vision.cv2_facade and vision.utils.{transform,color} refuse from their arguments alone (no
context, no GPU): wrong dtype, empty image, five channels, and each operator's own bad parameters.  tools/record_operator_refusals.py
records what every call raises into tests/golden/operator_refusals.json; tests/test_operator_layer.py asserts that it still does.

equalize_hist of the mirror is absent: it asks for the context before it looks at its argument, so what it raises without a GPU is
the missing device, not a refusal (its facade name, equalizeHist, refuses first and is here)."""
import numpy as np

U8 = np.zeros((7, 5), np.uint8)
BGR = np.zeros((7, 5, 3), np.uint8)
WRONG = np.zeros((7, 5), np.int32)                   # a dtype no operator here takes
EMPTY = np.zeros((0, 5), np.uint8)
FIVE = np.zeros((7, 5, 5), np.uint8)
MAPX = np.zeros((4, 6), np.float32)
EYE3 = np.eye(3)
CAMERA = np.array([[100.0, 0, 3], [0, 100.0, 2], [0, 0, 1]])


def cases():
    """[(id, call)]; every call raises"""
    from vision import cv2_facade as f
    from vision.utils import color as c
    from vision.utils import transform as t
    clahe = f.createCLAHE()
    wide = f.createCLAHE(2.0, (65, 8))
    # every operator that takes an image, as a function of the image alone: each gets the three bad images
    by_source = {
        "GaussianBlur": lambda s: f.GaussianBlur(s, (5, 5), 0),
        "simple_gaussian_blur": lambda s: t.simple_gaussian_blur(s, 5, 0),
        "medianBlur": lambda s: f.medianBlur(s, 3),
        "median_blur": lambda s: t.median_blur(s, 3),
        "equalizeHist": lambda s: f.equalizeHist(s),
        "CLAHE.apply": lambda s: clahe.apply(s),
        "Sobel": lambda s: f.Sobel(s, f.CV_16S, 1, 0),
        "sobel": lambda s: t.sobel(s, 1, 0),
        "Scharr": lambda s: f.Scharr(s, f.CV_16S, 1, 0),
        "scharr": lambda s: t.scharr(s, 1, 0),
        "Laplacian": lambda s: f.Laplacian(s, f.CV_16S),
        "laplacian": lambda s: t.laplacian(s),
        "spatialGradient": lambda s: f.spatialGradient(s),
        "spatial_gradient": lambda s: t.spatial_gradient(s),
        "convertScaleAbs": lambda s: f.convertScaleAbs(s),
        "convert_scale_abs": lambda s: t.convert_scale_abs(s),
        "boxFilter": lambda s: f.boxFilter(s, -1, (3, 3)),
        "box_filter": lambda s: t.box_filter(s, 3),
        "blur": lambda s: f.blur(s, (3, 3)),
        "box_blur": lambda s: t.box_blur(s, 3),
        "pyrDown": lambda s: f.pyrDown(s),
        "pyr_down": lambda s: t.pyr_down(s),
        "pyrUp": lambda s: f.pyrUp(s),
        "pyr_up": lambda s: t.pyr_up(s),
        "buildPyramid": lambda s: f.buildPyramid(s, 2),
        "build_pyramid": lambda s: t.build_pyramid(s, 2),
        "integral": lambda s: f.integral(s),
        "integral (mirror)": lambda s: t.integral(s),
        "warpAffine": lambda s: f.warpAffine(s, np.eye(2, 3), (5, 7)),
        "rotate": lambda s: t.rotate(s, 10.0),
        "translate": lambda s: t.translate(s, 1, 2),
        "remap": lambda s: f.remap(s, MAPX, MAPX, f.INTER_LINEAR),
        "remap (mirror)": lambda s: t.remap(s, MAPX, MAPX),
        "warpPerspective": lambda s: f.warpPerspective(s, EYE3, (5, 7)),
        "warp_perspective": lambda s: t.warp_perspective(s, EYE3, 5, 7),
        "resize": lambda s: f.resize(s, (4, 4)),
        "resize (mirror)": lambda s: t.resize(s, 4, 4),
        "undistort": lambda s: f.undistort(s, CAMERA, None),
    }
    out = []
    for name, call in by_source.items():
        for what, img in (("wrong dtype", WRONG), ("empty", EMPTY), ("five channels", FIVE)):
            out.append((f"{name}: {what}", lambda call=call, img=img: call(img)))
    out += [
        ("GaussianBlur: even kernel", lambda: f.GaussianBlur(U8, (4, 4), 0)),
        ("GaussianBlur: kernel above 511", lambda: f.GaussianBlur(U8, (513, 3), 0)),
        ("GaussianBlur: border", lambda: f.GaussianBlur(U8, (3, 3), 0, None, 0, f.BORDER_REPLICATE)),
        ("simple_gaussian_blur: even kernel", lambda: t.simple_gaussian_blur(U8, 4, 0)),
        ("medianBlur: even ksize", lambda: f.medianBlur(U8, 4)),
        ("medianBlur: ksize above 255", lambda: f.medianBlur(U8, 257)),
        ("medianBlur: ksize no integer", lambda: f.medianBlur(U8, "x")),
        ("medianBlur: two channels, ksize 7", lambda: f.medianBlur(np.zeros((7, 5, 2), np.uint8), 7)),
        ("median_blur: even ksize", lambda: t.median_blur(U8, 4)),
        ("median_blur: ksize above 255", lambda: t.median_blur(U8, 257)),
        ("Sobel: scale", lambda: f.Sobel(U8, f.CV_16S, 1, 0, scale=2)),
        ("Sobel: depth", lambda: f.Sobel(U8, f.CV_32S, 1, 0)),
        ("Sobel: even ksize", lambda: f.Sobel(U8, f.CV_16S, 1, 0, ksize=4)),
        ("Sobel: border", lambda: f.Sobel(U8, f.CV_16S, 1, 0, borderType=f.BORDER_WRAP)),
        ("Sobel: no order", lambda: f.Sobel(U8, f.CV_16S, 0, 0)),
        ("Sobel: third order", lambda: f.Sobel(U8, f.CV_16S, 3, 0, ksize=5)),
        ("sobel: depth", lambda: t.sobel(U8, 1, 0, 3, 4)),
        ("sobel: even ksize", lambda: t.sobel(U8, 1, 0, 4)),
        ("sobel: border", lambda: t.sobel(U8, 1, 0, 3, border=3)),
        ("Scharr: both orders", lambda: f.Scharr(U8, f.CV_16S, 1, 1)),
        ("Scharr: delta", lambda: f.Scharr(U8, f.CV_16S, 1, 0, delta=1)),
        ("scharr: both orders", lambda: t.scharr(U8, 1, 1)),
        ("Laplacian: even ksize", lambda: f.Laplacian(U8, f.CV_16S, ksize=2)),
        ("Laplacian: depth", lambda: f.Laplacian(U8, 7)),
        ("laplacian: even ksize", lambda: t.laplacian(U8, 2)),
        ("spatialGradient: ksize", lambda: f.spatialGradient(U8, ksize=5)),
        ("spatialGradient: border", lambda: f.spatialGradient(U8, borderType=f.BORDER_REFLECT)),
        ("spatialGradient: three channels", lambda: f.spatialGradient(BGR)),
        ("spatial_gradient: ksize", lambda: t.spatial_gradient(U8, 5)),
        ("spatial_gradient: border", lambda: t.spatial_gradient(U8, 3, 2)),
        ("spatial_gradient: three channels", lambda: t.spatial_gradient(BGR)),
        ("convertScaleAbs: alpha", lambda: f.convertScaleAbs(U8, None, 2)),
        ("convertScaleAbs: beta", lambda: f.convertScaleAbs(U8, None, 1, 3)),
        ("boxFilter: ksize 0", lambda: f.boxFilter(U8, -1, (0, 3))),
        ("boxFilter: ksize no pair", lambda: f.boxFilter(U8, -1, 3)),
        ("boxFilter: anchor", lambda: f.boxFilter(U8, -1, (3, 3), None, (0, 0))),
        ("boxFilter: window above 255", lambda: f.boxFilter(U8, -1, (256, 3))),
        ("boxFilter: normalised int16", lambda: f.boxFilter(U8, f.CV_16S, (3, 3))),
        ("boxFilter: depth", lambda: f.boxFilter(U8, 7, (3, 3), normalize=False)),
        ("boxFilter: border", lambda: f.boxFilter(U8, -1, (3, 3), borderType=f.BORDER_WRAP)),
        ("box_filter: window above 255", lambda: t.box_filter(U8, 256)),
        ("box_filter: normalised int16", lambda: t.box_filter(U8, 3, 3, 3)),
        ("box_filter: border", lambda: t.box_filter(U8, 3, border=3)),
        ("blur: ksize 0", lambda: f.blur(U8, (3, 0))),
        ("blur: anchor", lambda: f.blur(U8, (3, 3), None, (2, 2))),
        ("blur: border", lambda: f.blur(U8, (3, 3), borderType=f.BORDER_WRAP)),
        ("box_blur: window 0", lambda: t.box_blur(U8, 0)),
        ("pyrDown: dstsize", lambda: f.pyrDown(U8, None, (1, 1))),
        ("pyrDown: border", lambda: f.pyrDown(U8, borderType=f.BORDER_CONSTANT)),
        ("pyr_down: border", lambda: t.pyr_down(U8, 0)),
        ("pyrUp: dstsize", lambda: f.pyrUp(U8, None, (1, 1))),
        ("pyrUp: border", lambda: f.pyrUp(U8, borderType=f.BORDER_REPLICATE)),
        ("pyr_up: border", lambda: t.pyr_up(U8, 1)),
        ("buildPyramid: negative levels", lambda: f.buildPyramid(U8, -1)),
        ("build_pyramid: negative levels", lambda: t.build_pyramid(U8, -1)),
        ("integral: sdepth", lambda: f.integral(U8, None, f.CV_64F)),
        ("integral2", lambda: f.integral2(U8)),
        ("warpAffine: nearest", lambda: f.warpAffine(U8, np.eye(2, 3), (5, 7), None, f.INTER_NEAREST)),
        ("warpAffine: border", lambda: f.warpAffine(U8, np.eye(2, 3), (5, 7), borderMode=f.BORDER_REFLECT)),
        ("warpAffine: 3x3 matrix", lambda: f.warpAffine(U8, EYE3, (5, 7))),
        ("warpAffine: size", lambda: f.warpAffine(U8, np.eye(2, 3), (0, 7))),
        ("remap: interpolation", lambda: f.remap(U8, MAPX, MAPX, 2)),
        ("remap: border", lambda: f.remap(U8, MAPX, MAPX, f.INTER_LINEAR, None, f.BORDER_REFLECT)),
        ("remap: maps", lambda: f.remap(U8, MAPX.astype(np.float64), MAPX, f.INTER_LINEAR)),
        ("remap: int16 plane alone, linear", lambda: f.remap(U8, np.zeros((4, 6, 2), np.int16), None, f.INTER_LINEAR)),
        ("remap (mirror): border", lambda: t.remap(U8, MAPX, MAPX, border=2)),
        ("remap (mirror): maps", lambda: t.remap(U8, MAPX, None)),
        ("remap (mirror): fraction plane, nearest", lambda: t.remap(U8, np.zeros((4, 6, 2), np.int16), np.zeros((4, 6), np.uint16), True)),
        ("warpPerspective: interpolation", lambda: f.warpPerspective(U8, EYE3, (5, 7), None, 2)),
        ("warpPerspective: border", lambda: f.warpPerspective(U8, EYE3, (5, 7), borderMode=f.BORDER_REFLECT)),
        ("warpPerspective: dsize", lambda: f.warpPerspective(U8, EYE3, None)),
        ("warpPerspective: 2x3 matrix", lambda: f.warpPerspective(U8, np.eye(2, 3), (5, 7))),
        ("warpPerspective: size", lambda: f.warpPerspective(U8, EYE3, (0, 7))),
        ("warp_perspective: 2x3 matrix", lambda: t.warp_perspective(U8, np.eye(2, 3), 5, 7)),
        ("warp_perspective: size", lambda: t.warp_perspective(U8, EYE3, 5, 0)),
        ("warp_perspective: matrix not finite", lambda: t.warp_perspective(U8, np.full((3, 3), np.inf), 5, 7)),
        ("resize: interpolation", lambda: f.resize(U8, (4, 4), interpolation=f.INTER_NEAREST)),
        ("resize: neither dsize nor scales", lambda: f.resize(U8, None)),
        ("resize: negative scale", lambda: f.resize(U8, (0, 0), fx=-1, fy=2)),
        ("resize: size", lambda: f.resize(U8, (0, 4))),
        ("resize (mirror): size", lambda: t.resize(U8, 4, 0)),
        ("undistort: camera matrix", lambda: f.undistort(U8, np.eye(2), None)),
        ("undistort: coefficients", lambda: f.undistort(U8, CAMERA, [0.1, 0.2, 0.3])),
        ("initUndistortRectifyMap: m1type", lambda: f.initUndistortRectifyMap(CAMERA, None, None, CAMERA, (5, 7), f.CV_16UC1)),
        ("initUndistortRectifyMap: camera matrix", lambda: f.initUndistortRectifyMap(CAMERA * np.nan, None, None, CAMERA, (5, 7), f.CV_32FC1)),
        ("initUndistortRectifyMap: thin prism", lambda: f.initUndistortRectifyMap(CAMERA, [0.0] * 8 + [0.1] * 4, None, CAMERA, (5, 7), f.CV_32FC1)),
        ("initUndistortRectifyMap: size", lambda: f.initUndistortRectifyMap(CAMERA, None, None, CAMERA, (0, 7), f.CV_32FC1)),
        ("initUndistortRectifyMap: R", lambda: f.initUndistortRectifyMap(CAMERA, None, np.eye(2), CAMERA, (5, 7), f.CV_32FC1)),
        ("initUndistortRectifyMap: singular", lambda: f.initUndistortRectifyMap(CAMERA, None, None, np.zeros((3, 3)), (5, 7), f.CV_32FC1)),
        ("undistorter: camera matrix", lambda: t.undistorter(np.eye(2), None, (5, 7))),
        ("undistorter: coefficients", lambda: t.undistorter(CAMERA, [0.1, 0.2, 0.3], (5, 7))),
        ("undistorter: size", lambda: t.undistorter(CAMERA, None, (5, 0))),
        ("equalizeHist: three channels", lambda: f.equalizeHist(BGR)),
        ("CLAHE.apply: three channels", lambda: clahe.apply(BGR)),
        ("CLAHE.apply: more than 64 tiles", lambda: wide.apply(U8)),
        ("createCLAHE: grid", lambda: f.createCLAHE(2.0, (0, 8))),
        ("createCLAHE: clip limit", lambda: f.createCLAHE("x")),
        ("clahe: grid", lambda: c.clahe(U8, 2.0, (0, 8))),
        ("clahe: clip limit", lambda: c.clahe(U8, float("nan"))),
        ("clahe: grid no pair", lambda: c.clahe(U8, 2.0, 8)),
    ]
    return out


def outcome(call):
    """(exception class name, message) of a call, or None when it returns"""
    try:
        call()
    except Exception as e:  # noqa: BLE001  (whatever it raises is what is recorded)
        return [type(e).__name__, str(e)]
    return None
