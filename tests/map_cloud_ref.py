"""The three map scans of MapROS (plan_env/src/map_ros.cpp) restated in numpy over an f64 occupancy array [nx, ny, nz]
and an inflate array of the same shape: what fuelmi_map_extract_cloud must return, bit for bit.

  publishMapAll    :220-233  occ > min_occupancy_log, truncation, point;  :246-251  occ > clamp_min_log - 1e-3, counted
  publishMapLocal  :269-283  the same selection and point over the local box (:284-298, commented out there: inflate == 1)
  publishUnknown   :325-337  occ < clamp_min_log - 1e-3

All loop x outermost, then y, then z.  A selected voxel is dropped by the two `continue`s (:226-227, :276-277, :331-332):
pos(2) > visualization_truncate_height_ or pos(2) < visualization_truncate_low_, pos = indexToPos (sdf_map.h:132-135:
(id + 0.5) * resolution + origin per axis, f64).  pcl::PointXYZ holds floats: pt.x = pos(0) rounds each f64 once.

map_ros.cpp's publishers are not reachable through the oracle's exports; this restatement is pinned by reading.  `extract`
is the vectorised form the tests use, `extract_loop` the literal triple loop it is checked against on small boxes."""
import math

import numpy as np

OCCUPIED, UNKNOWN, KNOWN, INFLATED = range(4)
KINDS = (OCCUPIED, UNKNOWN, KNOWN, INFLATED)
KIND_NAMES = ("occupied", "unknown", "known", "inflated")


def logit(p):
    return math.log(p / (1 - p))  # SDFMap::initMap's logit (sdf_map.cpp:49-54)


class Params:
    """resolution, origin [3], min_occupancy_log, clamp_min_log of a map"""

    def __init__(self, res, origin, min_occupancy_log, clamp_min_log):
        self.res, self.origin = float(res), np.asarray(origin, dtype=np.float64)
        self.min_occupancy_log, self.clamp_min_log = float(min_occupancy_log), float(clamp_min_log)
        self.unknown_thr = self.clamp_min_log - 1e-3  # the literal of :249 and :328


def select(P, occ3, infl3, kind, known_as="reference"):
    """the boolean selection of a kind.  known_as: "reference" is :249's occ > thr, "plane" the complement of the unknown
    plane the device holds, !(occ < thr); they differ only for occ == thr or NaN"""
    if kind == OCCUPIED:
        return occ3 > P.min_occupancy_log
    if kind == UNKNOWN:
        return occ3 < P.unknown_thr
    if kind == KNOWN:
        return occ3 > P.unknown_thr if known_as == "reference" else ~(occ3 < P.unknown_thr)
    if kind == INFLATED:
        return infl3 == 1
    raise ValueError(kind)


def index_to_pos(P, idx):
    """indexToPos for an integer array [..., 3] (or one axis with `axis`)"""
    return (np.asarray(idx, dtype=np.float64) + 0.5) * P.res + P.origin


def axis_pos(P, i, axis):
    return (np.asarray(i, dtype=np.float64) + 0.5) * P.res + P.origin[axis]


def extract(P, occ3, infl3, kind, lo, hi, z_low=-np.inf, z_high=np.inf, known_as="reference"):
    """float32 [n, 3]: the cloud of the inclusive box lo..hi in loop order.  lo > hi on an axis: the loops do not run"""
    if any(lo[k] > hi[k] for k in range(3)):
        return np.zeros((0, 3), dtype=np.float32)
    sl = tuple(slice(lo[k], hi[k] + 1) for k in range(3))
    sel = select(P, occ3[sl], infl3[sl], kind, known_as)
    idx = np.argwhere(sel) + np.asarray(lo)  # C order: x outermost, then y, then z
    pos = index_to_pos(P, idx)
    with np.errstate(invalid="ignore"):
        keep = ~(pos[:, 2] > z_high) & ~(pos[:, 2] < z_low)
    return pos[keep].astype(np.float32)


def extract_loop(P, occ3, infl3, kind, lo, hi, z_low=-np.inf, z_high=np.inf, known_as="reference"):
    """the literal loops"""
    out = []
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                if not select(P, occ3[x, y, z], infl3[x, y, z], kind, known_as):
                    continue
                pos = [(i + 0.5) * P.res + P.origin[a] for a, i in enumerate((x, y, z))]
                if pos[2] > z_high:
                    continue
                if pos[2] < z_low:
                    continue
                out.append([np.float32(v) for v in pos])
    return np.array(out, dtype=np.float32).reshape(-1, 3)


def count(P, occ3, infl3, kind, lo, hi, z_low=-np.inf, z_high=np.inf, known_as="reference"):
    return len(extract(P, occ3, infl3, kind, lo, hi, z_low, z_high, known_as))


def inflate(P, occ3, step):
    """clearAndInflateLocalMap over the whole map (sdf_map.cpp:434-461): every voxel with occ > min_occupancy_log marks the
    cube of +-step voxels around it, each through toAddress() and kept iff 0 <= address < N"""
    nx, ny, nz = occ3.shape
    src = np.argwhere(occ3 > P.min_occupancy_log)
    r = np.arange(-step, step + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = (src[:, None, :] + off[None, :, :]).reshape(-1, 3)
    adr = (pts[:, 0] * ny + pts[:, 1]) * nz + pts[:, 2]
    adr = adr[(adr >= 0) & (adr < nx * ny * nz)]
    out = np.zeros(nx * ny * nz, dtype=np.int8)
    out[adr] = 1
    return out.reshape(occ3.shape)
