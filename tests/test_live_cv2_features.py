"""Live comparison of tests/features_restate.py with a real OpenCV's FAST detector and brute-force Hamming matcher.  Skipped where `cv2`
is not importable.  CPU-only.  This is the only place where the parity of the FAST score formula and of the matcher's distances with
OpenCV itself is checked: until it has run somewhere, the score formula and the tie order are this library's
stated definitions.  The descriptor has no counterpart in cv2 and is not compared."""
import numpy as np
import pytest

import features_cases as K
import features_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _images():
    yield "noise", K.noise(47, 61, 3)
    yield "scene", K.scene()[1]
    yield "dot", K.dot_image(200)
    yield "arc9", K.arc_image(12, 9, 40)
    yield "twins", K.twin_dots()


@pytest.mark.parametrize("nonmax", [True, False])
@pytest.mark.parametrize("threshold", [5, 20, 60])
def test_fast_points_and_responses_are_cv2s(threshold, nonmax):
    for name, img in _images():
        det = cv2.FastFeatureDetector_create(threshold, nonmax, cv2.FAST_FEATURE_DETECTOR_TYPE_9_16)
        kps = det.detect(np.ascontiguousarray(img), None)
        got = sorted((int(k.pt[1]), int(k.pt[0]), int(k.response)) for k in kps)
        xy, score = R.fast(img, threshold, nonmax)
        want = sorted((int(y), int(x), int(s)) for (x, y), s in zip(xy, score))
        assert got == want, (name, threshold, nonmax, len(got), len(want))


@pytest.mark.parametrize("D", [8, 32, 64])
def test_knn_distances_are_cv2s_and_indices_where_they_are_decided(D):
    q, t = np.ascontiguousarray(K.descriptors(65, D, 1)), np.ascontiguousarray(K.descriptors(257, D, 2))
    idx, dist = R.hamming_knn(q, t, 2)
    d = R.hamming_matrix(q, t)
    matches = cv2.BFMatcher(cv2.NORM_HAMMING).knnMatch(q, t, k=2)
    for i, pair in enumerate(matches):
        assert [int(m.distance) for m in pair] == dist[i].tolist(), i
        if (d[i] == dist[i, 0]).sum() == 1 and (d[i] == dist[i, 1]).sum() == 1:        # the two best distances are unique in the row
            assert [m.trainIdx for m in pair] == idx[i].tolist(), i
