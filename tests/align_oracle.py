"""Oracle of the face alignment (K13c and its host side): scikit-image's Umeyama estimate per face, and
``cv2.warpAffine(img, M, (112, 112), flags=INTER_LINEAR, borderValue=0)`` restated in numpy int64.

**Parity unpinned**: neither cv2 nor scikit-image is installed where this suite runs, so both are restatements of the
published sources [PUBLIC-LIB] (``skimage/transform/_geometric.py::_umeyama``, OpenCV ``imgproc/imgwarp.cpp``
``warpAffine`` / ``WarpAffineInvoker`` / ``remapBilinear``); ``tests/test_face_align_host.py`` compares them with the real
libraries wherever those can be imported.
"""
from __future__ import annotations

import numpy as np

import face_oracle as fo
from eioku_amd import faces

AB_BITS, INTER_BITS = 10, 5
AB_SCALE, INTER_TAB_SIZE = 1 << AB_BITS, 1 << INTER_BITS


# ---- skimage.transform._geometric._umeyama(src, dst, estimate_scale=True), one face -------------------------------------
def umeyama(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """``(N, 2)`` source and destination points -> the homogeneous ``(3, 3)`` similarity (NaN when the rank is 0)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=np.float64)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.float64)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    elif rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    with np.errstate(all="ignore"):
        scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T


def estimate(landmarks_xy: np.ndarray) -> np.ndarray:
    """insightface ``estimate_norm``: ``SimilarityTransform.estimate(landmarks, arcface_dst).params[:2]`` per face."""
    return np.stack([umeyama(l, faces.ARCFACE_DST)[:2] for l in np.asarray(landmarks_xy, np.float64).reshape(-1, 5, 2)])


# ---- cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT 0, 8-bit ----------------------------------------------------------
def rne(v) -> np.ndarray:
    """``cvRound`` / ``saturate_cast<int>(double)``: round half to even, saturating at int32; NaN -> 0."""
    with np.errstate(all="ignore"):
        v = np.rint(np.asarray(v, np.float64))
        v = np.where(np.isnan(v), 0.0, v)
        return np.clip(v, -2147483648.0, 2147483647.0).astype(np.int64)


def invert(M) -> np.ndarray:
    """warpAffine's own inversion of the forward matrix (no WARP_INVERSE_MAP), float64, every operation rounded."""
    M0, M1, M2, M3, M4, M5 = (np.float64(v) for v in np.asarray(M, np.float64).reshape(6))
    with np.errstate(all="ignore"):
        D = M0 * M4 - M1 * M3
        D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
        A11, A22 = M4 * D, M0 * D
        M0 = A11
        M1 = M1 * -D
        M3 = M3 * -D
        M4 = A22
        b1 = -M0 * M2 - M1 * M5
        b2 = -M3 * M2 - M4 * M5
    return np.array([M0, M1, b1, M3, M4, b2], np.float64)


def warp_one(frame_bgr: np.ndarray, M, size: int = faces.CROP) -> np.ndarray:
    """One ``(size, size, 3)`` uint8 BGR image: the four steps of K13c, literally."""
    h, w, _ = frame_bgr.shape
    iM = invert(M)
    x = np.arange(size, dtype=np.float64)
    y = np.arange(size, dtype=np.float64)
    with np.errstate(all="ignore"):
        adelta, bdelta = rne(iM[0] * x * AB_SCALE), rne(iM[3] * x * AB_SCALE)
        X0 = rne((iM[1] * y + iM[2]) * AB_SCALE) + AB_SCALE // INTER_TAB_SIZE // 2
        Y0 = rne((iM[4] * y + iM[5]) * AB_SCALE) + AB_SCALE // INTER_TAB_SIZE // 2
    X = (X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx, sy = np.clip(X >> INTER_BITS, -32768, 32767), np.clip(Y >> INTER_BITS, -32768, 32767)
    fx, fy = X & (INTER_TAB_SIZE - 1), Y & (INTER_TAB_SIZE - 1)
    f = frame_bgr.astype(np.int64)
    acc = np.full((size, size, 3), 512, np.int64)
    for dy, wy in ((0, INTER_TAB_SIZE - fy), (1, fy)):
        for dx, wx in ((0, INTER_TAB_SIZE - fx), (1, fx)):
            yy, xx = sy + dy, sx + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            px = f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            acc += np.where(ok[..., None], (wy * wx)[..., None] * px, 0)
    return (acc >> 10).astype(np.uint8)


def warp_u8(frames_bgr: np.ndarray, slots, M) -> np.ndarray:
    """``(m,112,112,3)`` uint8 **RGB** crops (``face_oracle.crop_u8``'s layout) of frames ``slots`` under matrices ``M``."""
    mats = np.asarray(M, np.float64).reshape(-1, 6)
    return np.stack([warp_one(frames_bgr[int(s)], m)[..., ::-1] for s, m in zip(slots, mats)])


def warp_input(frames_bgr, slots, M) -> np.ndarray:
    """What K13c writes: fp16 NHWC8."""
    return fo.normalise(warp_u8(frames_bgr, slots, M))
