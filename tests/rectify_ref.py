"""float64 numpy restatement of the rectification ops (include/einx.h), written from the camera models: the
equidistant fisheye model with a four-term polynomial in the incidence angle, and the radial-tangential (Brown-Conrady) model
with three radial and two tangential coefficients.  OpenCV is not among the test dependencies, so nothing here is checked
against it; the tests compare the kernels with THESE definitions.

Every expression is written in the operation order the header gives, so that the kernels (float64, no contraction) can only
differ from it through the last-place differences of atan / sqrt and a double rounding on the way to float32."""
import numpy as np

# calibrations of the magnitude the two datasets ship (data, not code)
EC_K = (199.0924, 198.8288, 132.1921, 110.7127)
EC_D = (-0.368436, 0.150947, -0.000296, -0.000439, 0.0)
EC_SIZE = (240, 180)  # (W, H)
MVSEC_K = (226.38, 226.15, 173.65, 133.73)
MVSEC_D = (-0.048, 0.0113, -0.0553, 0.0399)
MVSEC_SIZE = (346, 260)
_a = 0.01
MVSEC_R = np.array([[np.cos(_a), 0.0, np.sin(_a)], [0.0, 1.0, 0.0], [-np.sin(_a), 0.0, np.cos(_a)]])
MVSEC_P = np.array([[199.65, 0.0, 177.4, 0.0], [0.0, 199.65, 126.8, 0.0], [0.0, 0.0, 1.0, 0.0]])
SMALL_SIZE = (13, 7)
IDENTITY_K = (1.0, 1.0, 0.0, 0.0)


def camera_matrix(K):
    fx, fy, cx, cy = K
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _grid(size):
    W, H = size
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return u, v


def inverse3(a):
    """the adjugate over the determinant, element by element as the library's host code does (numpy.linalg.inv goes through an LU
    factorisation and differs in the last place)"""
    a = np.asarray(a, np.float64).reshape(9)
    c0 = a[4] * a[8] - a[5] * a[7]
    c1 = a[5] * a[6] - a[3] * a[8]
    c2 = a[3] * a[7] - a[4] * a[6]
    det = a[0] * c0 + a[1] * c1 + a[2] * c2
    return np.array([c0 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                     c1 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                     c2 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det])


def _pr(P, R):
    P, R = np.asarray(P, np.float64)[:, :3], np.asarray(R, np.float64)
    out = np.empty(9)
    for i in range(3):
        for j in range(3):
            out[3 * i + j] = P[i, 0] * R[0, j] + P[i, 1] * R[1, j] + P[i, 2] * R[2, j]
    return out


def _back_project(P, R, size):
    m = inverse3(_pr(P, R))
    u, v = _grid(size)
    X = m[0] * u + m[1] * v + m[2]
    Y = m[3] * u + m[4] * v + m[5]
    Wd = m[6] * u + m[7] * v + m[8]
    with np.errstate(all="ignore"):
        return X / Wd, Y / Wd, Wd


def radtan_terms(D, x, y):
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x))
    dy = p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y
    return kr, dx, dy


def fisheye_map(K, D, R, P, size):
    """(map_x, map_y) in float64: the equidistant model, theta_d = theta (1 + k1 theta^2 + ... + k4 theta^8)"""
    fx, fy, cx, cy = K
    x, y, Wd = _back_project(P, R, size)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        th = np.arctan(r)
        th2 = th * th
        th4 = th2 * th2
        th6 = th4 * th2
        th8 = th4 * th4
        thd = th * (1.0 + D[0] * th2 + D[1] * th4 + D[2] * th6 + D[3] * th8)
        s = np.where(r == 0.0, 1.0, thd / np.where(r == 0.0, 1.0, r))
        mx = fx * x * s + cx
        my = fy * y * s + cy
    bad = Wd <= 0.0
    return np.where(bad, -1.0, mx), np.where(bad, -1.0, my)


def radtan_map(K, D, size, R=None, P=None):
    fx, fy, cx, cy = K
    R = np.eye(3) if R is None else R
    P = camera_matrix(K) if P is None else P
    x, y, _ = _back_project(P, R, size)
    with np.errstate(all="ignore"):
        kr, dx, dy = radtan_terms(D, x, y)
        return fx * (x * kr + dx) + cx, fy * (y * kr + dy) + cy


def undistort_points(K, D, u, v, P=None, iters=5):
    """float64 positions of the raw pixels (u, v) after `iters` fixed-point steps and the projection with P (None: K)"""
    fx, fy, cx, cy = K
    P = np.asarray(camera_matrix(K) if P is None else P, np.float64)[:, :3]
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    with np.errstate(all="ignore"):
        for _ in range(iters):
            kr, dx, dy = radtan_terms(D, x, y)
            x, y = (x0 - dx) / kr, (y0 - dy) / kr
        X = P[0, 0] * x + P[0, 1] * y + P[0, 2]
        Y = P[1, 0] * x + P[1, 1] * y + P[1, 2]
        Wp = P[2, 0] * x + P[2, 1] * y + P[2, 2]
        return X / Wp, Y / Wp


def undistort_points_map(K, D, size, P=None, iters=5, rint=True):
    u, v = _grid(size)
    mx, my = undistort_points(K, D, u, v, P, iters)
    return (np.rint(mx), np.rint(my)) if rint else (mx, my)


def distort_points(K, D, xu, yu):
    """the forward radtan model: undistorted PIXEL positions (projected with K) -> raw pixel positions"""
    fx, fy, cx, cy = K
    x, y = (xu - cx) / fx, (yu - cy) / fy
    kr, dx, dy = radtan_terms(D, x, y)
    return fx * (x * kr + dx) + cx, fy * (y * kr + dy) + cy


def remap(src, map_x, map_y):
    """bilinear sampling in float64: src [F, Hs, Ws] (any real type), maps [H, W] -> float64 [F, H, W]; taps outside the source
    read 0, a map entry that is not finite gives 0"""
    src = np.asarray(src, np.float64)
    F, Hs, Ws = src.shape
    mx, my = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
    ok = np.isfinite(mx) & np.isfinite(my) & (mx > -1) & (mx < Ws) & (my > -1) & (my < Hs)
    mxs, mys = np.where(ok, mx, 0.0), np.where(ok, my, 0.0)
    x0, y0 = np.floor(mxs), np.floor(mys)
    fx, fy = mxs - x0, mys - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
        return np.where(inside[None], src[:, np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)], 0.0)

    i00, i01, i10, i11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = i00 + fx * (i01 - i00)
    bot = i10 + fx * (i11 - i10)
    return np.where(ok[None], top + fy * (bot - top), 0.0)


def rectify_events(x, y, t, p, map_x, map_y, x_hi, y_hi):
    """the numpy form of the event pass on float32 x / y / p and float64 t: (x', y', t, p, kept, outside).  Events whose rounded
    raw coordinate is no pixel of the map (or is not finite) are counted in `outside` and dropped, never wrapped."""
    x, y, p = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(p, np.float32)
    t = np.asarray(t, np.float64)
    H, W = map_x.shape
    with np.errstate(all="ignore"):
        ox, oy = np.round(x), np.round(y)  # half to even
        inside = (ox >= 0) & (ox < W) & (oy >= 0) & (oy < H)  # NaN and inf fail
        oxi = np.where(inside, ox, 0).astype(np.int64)
        oyi = np.where(inside, oy, 0).astype(np.int64)
        rx, ry = map_x[oyi, oxi], map_y[oyi, oxi]
        keep = inside & (rx >= 0) & (rx < np.float32(x_hi)) & (ry >= 0) & (ry < np.float32(y_hi))
    return rx[keep], ry[keep], t[keep], p[keep], int(keep.sum()), int((~inside).sum())
