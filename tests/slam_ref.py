"""Long-double restatement of the rows of a SLAM landmark that is already in the state (np_ref.feature_jacobian_full with the
landmark's own first estimate, update/UpdaterHelper.cpp:195-513, and the point-on-plane row with the plane as a state variable,
:448-512), with the rounding bound of every element: the truth of tests/slam_precision_cases.py, as tests/propagate_ref.py is the
IMU's.

One set of functions, written over a number type.  Run on floats it is a plain float64 model; run on `E` it is the truth and
its companion at once.  E(v, e) carries the long-double value v and e, a bound in units of u on what one rounding per operation
leaves of error in v to first order - the running form of "the same expression with |.| of every operand":
  a + b   e_a + e_b + |v|            a * b   |a| e_b + |b| e_a + |v|          a / b   e_a / |b| + |a| e_b / b^2 + |v|
  sqrt a  e_a / (2 v) + |v|          atan a  e_a / (1 + a^2) + 2 |v|  (a 2 ulp arctangent)
  ssum    sum e_i + (k - 1) sum |v_i|: a k-term sum in ANY order of association, fused or not
so a difference of nearly equal values (the equidistant lens' dc/dr, the plane row's p - (n.p) n - d n) is charged with the
operands' size, not the result's.  Inputs (the scene's doubles, the float32 pixels) are exact: e = 0, and nothing is rounded before
the end.  A constant element (a 0 or a 1 of the intrinsics' block before whitening, a column the row does not touch) has e = 0.
"""
import numpy as np

from oracle import ld_ref

LD = ld_ref.LD


class E:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = LD(v)
        self.e = LD(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        o = E.of(o)
        v = self.v + o.v
        return E(v, self.e + o.e + abs(v))

    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        v = self.v - o.v
        return E(v, self.e + o.e + abs(v))

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        v = self.v * o.v
        return E(v, abs(self.v) * o.e + abs(o.v) * self.e + abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        return E(v, self.e / abs(o.v) + abs(self.v) * o.e / (o.v * o.v) + abs(v))

    def __rtruediv__(self, o):
        return E.of(o) / self


def ssum(ts):
    """a sum in any order of association"""
    if not any(isinstance(t, E) for t in ts):
        return sum(ts)
    ts = [E.of(t) for t in ts]
    return E(sum(t.v for t in ts), sum(t.e for t in ts) + (len(ts) - 1) * sum(abs(t.v) for t in ts))


def sqrt(a):
    if not isinstance(a, E):
        return np.sqrt(a)
    v = np.sqrt(a.v)
    return E(v, a.e / (2 * v) + v)


def atan(a):
    if not isinstance(a, E):
        return np.arctan(a)
    v = np.arctan(a.v)
    return E(v, a.e / (1 + a.v * a.v) + 2 * abs(v))


def dot(a, b):
    return ssum([x * y for x, y in zip(a, b)])


def quat_2_rot(q):
    """JPL: (2 q4^2 - 1) I - 2 q4 [qv]x + 2 qv qv^T, rows of a 3 x 3"""
    x, y, z, w = q
    a = 2 * w * w - 1
    return [[a + 2 * x * x, 2 * w * z + 2 * x * y, -(2 * w * y) + 2 * x * z],
            [-(2 * w * z) + 2 * y * x, a + 2 * y * y, 2 * w * x + 2 * y * z],
            [2 * w * y + 2 * z * x, -(2 * w * x) + 2 * z * y, a + 2 * z * z]]


def _radtan(x, y, v):
    """(distorted pixel, dz_dzn [2][2], dz_dzeta [2][8]) of ext CamRadtan"""
    fx, fy, cx, cy, k1, k2, p1, p2 = v
    r2 = x * x + y * y
    r4 = r2 * r2
    g = ssum([1, k1 * r2, k2 * r4])
    x1 = ssum([x * g, 2 * p1 * x * y, p2 * (r2 + 2 * x * x)])
    y1 = ssum([y * g, p1 * (r2 + 2 * y * y), 2 * p2 * x * y])
    off = ssum([2 * k1 * x * y, 4 * k2 * x * y * r2, 2 * p1 * x, 2 * p2 * y])
    dzn = [[fx * ssum([g, 2 * k1 * x * x, 4 * k2 * x * x * r2, 2 * p1 * y, 6 * p2 * x]), fx * off],
           [fy * off, fy * ssum([g, 2 * k1 * y * y, 4 * k2 * y * y * r2, 6 * p1 * y, 2 * p2 * x])]]
    dze = [[x1, 0, 1, 0, fx * x * r2, fx * x * r4, 2 * fx * x * y, fx * (r2 + 2 * x * x)],
           [0, y1, 0, 1, fy * y * r2, fy * y * r4, fy * (r2 + 2 * y * y), 2 * fy * x * y]]
    return (fx * x1 + cx, fy * y1 + cy), dzn, dze


def _equi(x, y, v):
    """the same of ext CamEqui (r > 1e-8 in every scene here)"""
    fx, fy, cx, cy, k1, k2, k3, k4 = v
    r2 = x * x + y * y
    r = sqrt(r2)
    th = atan(r)
    t2 = th * th
    th3 = th * t2
    th5 = th3 * t2
    th7 = th5 * t2
    th9 = th7 * t2
    th_d = ssum([th, k1 * th3, k2 * th5, k3 * th7, k4 * th9])
    cdist = th_d / r
    dthd_dr = ssum([1, 3 * k1 * t2, 5 * k2 * t2 * t2, 7 * k3 * t2 * t2 * t2, 9 * k4 * t2 * t2 * t2 * t2]) / (1 + r2)
    dc_dr = (dthd_dr * r - th_d) / r2
    s = dc_dr / r
    d = [[cdist + x * x * s, x * y * s], [x * y * s, cdist + y * y * s]]
    dzn = [[fx * d[0][0], fx * d[0][1]], [fy * d[1][0], fy * d[1][1]]]
    qx, qy = fx * x / r, fy * y / r
    dze = [[x * cdist, 0, 1, 0, qx * th3, qx * th5, qx * th7, qx * th9],
           [0, y * cdist, 0, 1, qy * th3, qy * th5, qy * th7, qy * th9]]
    return (fx * x * cdist + cx, fy * y * cdist + cy), dzn, dze


def bearing_rows(cam, clone, clone_fej, p_f, p_fej, uv, white, do_fej):
    """The two rows of one observation.  cam = (calib_q, calib_p, intr, fisheye), clone = (q, p), clone_fej the same at the first
    estimate, p_f / p_fej the landmark's value and first estimate, uv the measured pixel.  Returns (res [2], H_f [2][3],
    H_clone [2][6], H_calib [2][6], H_intr [2][8])."""
    Rc = quat_2_rot(cam[0])
    pIC, intr = cam[1], cam[2]

    def chain(cl, pf):
        R = quat_2_rot(cl[0])
        d = [pf[k] - cl[1][k] for k in range(3)]
        pI = [dot(R[i], d) for i in range(3)]
        pC = [ssum([Rc[i][0] * pI[0], Rc[i][1] * pI[1], Rc[i][2] * pI[2], pIC[i]]) for i in range(3)]
        return R, pI, pC

    R, pI, pC = chain(clone, p_f)
    x, y = pC[0] / pC[2], pC[1] / pC[2]
    (ud, vd), dzn, dze = (_equi if cam[3] else _radtan)(x, y, intr)  # at the value's uv_norm (:383, :389)
    res = [white * (uv[0] - ud), white * (uv[1] - vd)]
    if do_fej:
        R, pI, pC = chain(clone_fej, p_fej)
    z = pC[2]
    RcR = [[ssum([Rc[i][0] * R[0][k], Rc[i][1] * R[1][k], Rc[i][2] * R[2][k]]) for k in range(3)] for i in range(3)]
    RcS = [[Rc[i][1] * pI[2] - Rc[i][2] * pI[1], Rc[i][2] * pI[0] - Rc[i][0] * pI[2], Rc[i][0] * pI[1] - Rc[i][1] * pI[0]]
           for i in range(3)]  # R_ItoC skew(p_FinIi)
    q = [pC[k] - pIC[k] for k in range(3)]
    Hf, Hcl, Hca, Hin = [], [], [], []
    for r in range(2):
        zz = [dzn[r][0] / z, dzn[r][1] / z, -(dzn[r][0] * pC[0] + dzn[r][1] * pC[1]) / (z * z)]  # dz_dpfc
        hf = [white * ssum([zz[0] * RcR[0][k], zz[1] * RcR[1][k], zz[2] * RcR[2][k]]) for k in range(3)]
        th = [white * ssum([zz[0] * RcS[0][k], zz[1] * RcS[1][k], zz[2] * RcS[2][k]]) for k in range(3)]
        Hf.append(hf)
        Hcl.append(th + [-h for h in hf])
        Hca.append([white * (zz[1] * q[2] - zz[2] * q[1]), white * (zz[2] * q[0] - zz[0] * q[2]), white * (zz[0] * q[1] - zz[1] * q[0]),
                    white * zz[0], white * zz[1], white * zz[2]])
        Hin.append([white * e for e in dze[r]])
    return res, Hf, Hcl, Hca, Hin


def plane_row(p_f, p_fej, cp, cp_fej, white_c, do_fej):
    """(res, H_f [3], H_plane [3]) of the point-on-plane row, the plane a state variable (:448-512)"""
    d = sqrt(dot(cp, cp))
    n = [c / d for c in cp]
    res = white_c * (0 - (dot(n, p_f) - d))
    lp = p_f
    if do_fej:
        lp = p_fej
        d = sqrt(dot(cp_fej, cp_fej))
        n = [c / d for c in cp_fej]
    npv = dot(n, lp)
    s = white_c * 1 / d
    return res, [white_c * c for c in n], [s * ssum([lp[k], -(npv * n[k]), -(d * n[k])]) for k in range(3)]


# ---- a scene's landmark -----------------------------------------------------------------------------------------------------
def _tables(sc, num):
    cv = lambda a: [num(float(x)) for x in a]  # noqa: E731
    if "cams" in sc:
        cams = [(cv(t["calib_q"]), cv(t["calib_p"]), cv(t["intr"]), bool(t["fisheye"]), int(t["calib_id"]), int(t["intr_id"])) for t in sc.cams]
    else:
        fish = bool(sc.get("fisheye", False))
        cams = [(cv(sc.calib_q), cv(sc.calib_p), cv(sc.intr), fish, int(sc.ids["calib"]), int(sc.ids["intr"]))]
        if "cam1" in sc:
            c1 = sc.cam1
            cams.append((cv(c1["calib_q"]), cv(c1["calib_p"]), cv(c1["intr"]), False, int(sc.ids["calib1"]), int(sc.ids["intr1"])))
    return cams, cv


def landmark_rows(sc, f, plane=None, num=E, p_fej=None):
    """Rows of landmark f of a SLAM scene (synth.make_slam_scene / make_stereo_slam_scene / a `cams` scene) over the STATE's columns:
    2 per observation in observation order, then (plane = (state id, cp, cp_fej)) one point-on-plane row per observation.  Returns
    (H [rows, N], res [rows]) as arrays of `num` (E: truth and bound; float: the float64 model).  p_fej overrides the landmark's
    first estimate."""
    o = sc.opts
    cams, cv = _tables(sc, num)
    m = int(sc.n_meas[f])
    cam_of = sc.cam_idx[f, :m] if "cam_idx" in sc else np.zeros(m, dtype=np.int64)
    white = num(1.0 / o["sigma_px"])
    p_f = cv(sc.p_FinG[f])
    p_e = cv(sc.p_FinG_fej[f] if p_fej is None else p_fej)
    lm = int(sc.lm_id[f])
    rows = 2 * m + (m if plane is not None else 0)
    zero = num(0.0)
    H = np.full((rows, int(sc.N)), zero, dtype=object)
    res = np.full(rows, zero, dtype=object)
    for a in range(m):
        ci, cam = int(sc.clone_idx[f, a]), cams[int(cam_of[a])]
        r, Hf, Hcl, Hca, Hin = bearing_rows(cam, (cv(sc.clone_q[ci]), cv(sc.clone_p[ci])), (cv(sc.clone_q_fej[ci]), cv(sc.clone_p_fej[ci])),
                                            p_f, p_e, cv(sc.uv[f, a]), white, bool(o["do_fej"]))
        cid = int(sc.ids["clones"][ci])
        for k in range(2):
            i = 2 * a + k
            res[i] = r[k]
            H[i, lm:lm + 3] = Hf[k]
            H[i, cid:cid + 6] = Hcl[k]
            if o["do_calib_pose"]:
                H[i, cam[4]:cam[4] + 6] = Hca[k]
            if o["do_calib_intr"]:
                H[i, cam[5]:cam[5] + 8] = Hin[k]
    if plane is not None:
        sid, cp, cpf = plane
        r, hf, hc = plane_row(p_f, p_e, cv(cp), cv(cpf), num(1.0 / o["sigma_c"]), bool(o["do_fej"]))
        for a in range(m):
            i = 2 * m + a
            res[i] = r
            H[i, lm:lm + 3] = hf
            H[i, sid:sid + 3] = hc
    return H, res


def split(A):
    """(values, bounds in units of u) of an array of E; of floats (values, None)"""
    flat = A.reshape(-1)
    if not isinstance(flat[0], E):
        return np.array(flat, dtype=np.float64).reshape(A.shape), None
    v = np.array([x.v for x in flat], dtype=LD).reshape(A.shape)
    e = np.array([x.e for x in flat], dtype=LD).reshape(A.shape)
    return v, e
