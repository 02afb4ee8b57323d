"""Mirror of the reference utils/sift.py: the `SIFT` class interface - sources added by name, then every source found in a frame with
the quadrilateral its corners map to.

What the class is: single-scale binary features under the reference's interface.  FAST-9 corners, the library's steered 256-bit
descriptor, brute-force Hamming matching with the ratio test, then findHomography by RANSAC - all on the GPU
(vision.utils.feature: fast_corners, describe_points, match_descriptors, ratio_test, estimate_motion).
They tolerate in-plane rotation and small changes of scale.  They are not scale-invariant SIFT: there is no scale space, the
descriptors are 32 bytes of bits and not 128 floats, and a source seen at half or twice its size will not be found.

`PyramidSIFT` is the same class over a scale pyramid (vision.utils.feature.pyramid_features): the corners are
found and described on up to eight levels a factor 1.2 apart and reported in the coordinates of the image, so a source is also found
at half or twice its size - the property the reference's use (an object the vehicle drives towards) depends on.  Still binary
features, still not SIFT's scale space or its 128 floats."""
import numpy as np

from vision import cv2_facade as _cv2
from vision.utils import feature as _feature

MAX_POINTS = 2000          # corners described per image: the highest FAST scores
FAST_THRESHOLD = 20
RANSAC_THRESHOLD = 5.0     # utils/sift.py:117


class SIFT:
    """The reference's wrapper (utils/sift.py:5) over this library's features.  Images are uint8, single channel, numpy or DeviceMat."""

    def __init__(self, checks=50):
        """checks: the reference's FLANN parameter; accepted and unused - the matcher here is exhaustive."""
        self.sources = {}

    @staticmethod
    def _detect(img):
        """(keypoint list, descriptors (n, 32) uint8, positions (n, 2) float32) of the corners that can be described"""
        pts, scores = _feature.fast_corners(img, FAST_THRESHOLD, True, MAX_POINTS)
        kept, des, index = _feature.describe_points(img, pts)
        return _cv2.keypoints_of(kept, scores[index]), des, kept

    def add_source(self, name, source):
        """Adds an image as a source.  Returns its keypoints and descriptors."""
        kp, des, pts = self._detect(source)
        self.sources[name] = {"name": name, "source": source, "kp": kp, "des": des, "pts": pts}
        return kp, des

    def add_many(self, **kwargs):
        """Adds several sources: keyword = name, value = image."""
        for name, source in kwargs.items():
            self.add_source(name, source)

    def _ratio_test(matches, ratio=0.7):
        """utils/sift.py:60 on knnMatch's lists; pairs without a second neighbour are dropped (the reference's loop fails on them)"""
        return [m[0] for m in matches if len(m) == 2 and m[0].distance < ratio * m[1].distance]

    def match(self, img, min_match=10, ratio=0.7, draw=False):
        """Finds every source in `img`: ([(name, good matches, corners int32 (4, 1, 2), matchesMask list, None)], keypoints of img,
        descriptors of img).  The corners are those of the source - (0, 0), (0, h-1), (w-1, h-1), (w-1, 0) - under the homography.
        draw=True raises: drawMatches is not provided."""
        if draw:
            raise _cv2.error("SIFT.match: draw=True needs cv2.drawMatches, which is outside the accelerated path (DESIGN.md section 7)")
        kp, des, pts = self._detect(img)
        matched = []
        for name, val in self.sources.items():
            if len(val["des"]) == 0 or len(des) == 0:
                continue
            idx, dist = _feature.match_descriptors(val["des"], des, k=2)
            q, t = _feature.ratio_test(idx, dist, ratio)
            good = [_cv2.DMatch(int(a), int(b), 0, float(dist[a, 0])) for a, b in zip(q, t)]
            if len(good) < min_match or len(good) < 4:
                continue
            M, inliers = _feature.estimate_motion(val["pts"][q], pts[t], model="homography", threshold=RANSAC_THRESHOLD)
            if M is None:
                continue
            h, w = val["source"].shape[:2]
            corners = np.float32([[0, 0], [0, h - 1], [w - 1, h - 1], [w - 1, 0]]).reshape(-1, 1, 2)
            dst = np.int32(_cv2.perspectiveTransform(corners, M))
            matched.append((val["name"], good, dst, inliers.astype(np.uint8).tolist(), None))
        return matched, kp, des


class PyramidSIFT(SIFT):
    """SIFT's interface over pyramid_features: every image is searched on `levels` scales a factor 1.2 apart, each keypoint carries
    its level as `octave`, the patch's diameter in the image as `size` (31 w_0 / w_l) and its orientation bin as `angle` (11.25
    degrees a bin), and its position is in the image's own coordinates, so `match` maps the source's corners as before."""

    def __init__(self, checks=50, levels=8):
        """checks: as SIFT's, accepted and unused.  levels: pyramid levels asked for, 1 to 8."""
        super().__init__(checks)
        self.levels = int(levels)

    def _detect(self, img):
        """(keypoint list, descriptors (n, 32) uint8, positions (n, 2) float32 in the image's coordinates)"""
        pts, des, level, scores, bins = _feature.pyramid_features(img, FAST_THRESHOLD, MAX_POINTS, self.levels)
        w0 = img.shape[1]
        widths = [w for w, _ in _feature.pyramid_level_sizes(w0, img.shape[0], self.levels)]
        kp = [_cv2.KeyPoint(float(p[0]), float(p[1]), float(np.float32(31.0 * w0 / widths[l])), 11.25 * int(b), float(s), int(l), -1)
              for p, l, s, b in zip(pts, level, scores, bins)]
        return kp, des, pts
