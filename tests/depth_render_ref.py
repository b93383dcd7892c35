"""Restatement of the simulated depth camera (uav_simulator/local_sensing) that fuelmi_render_depth is compared with.

Two forms per model (include/fuelmi.h "Depth renderer" states the rules):
  literal_*   the node's loop over the cloud IN CLOUD ORDER with numpy scalar types: HOST_NODE is
              src/depth_render_node.cpp:126-161 including the `value < 1e-3` branch of the pixel update (:154-159),
              CUDA_NODE is src/depth_render.cu:8-42 (atomicMin on 999999) and src/pcl_render_node.cpp:300-310.  It does
              NOT drop a point nearer than 1e-3 (deviation 1): that is what the deviation scene shows.  It does skip the
              points of deviation 2, where the reference's conversions are undefined.
  project / render   the vectorised form the device is held to: every point's culls, window and 32-bit key from array
              arithmetic in the same types and order, then the minimum of the keys over the windows, 0xFFFFFFFF = empty.
Every f32 / f64 step is spelled with explicit numpy types (no Python-float promotion), so each expression rounds where the
source rounds; numpy does not contract.
"""
import numpy as np

HOST_NODE, CUDA_NODE = 0, 1
MODELS = (HOST_NODE, CUDA_NODE)
f32, f64 = np.float32, np.float64
EMPTY = np.uint32(0xFFFFFFFF)
# why a point is not (or is) splatted
KEPT, RANGE, BEHIND, OFFIMG, UNDEF_NONFINITE, UNDEF_NEAR, UNDEF_INT = range(7)
UNDEF = (UNDEF_NONFINITE, UNDEF_NEAR, UNDEF_INT)
TWO31 = 2147483648.0


class Cam:
    def __init__(self, rows, cols, fx, fy, cx, cy, model, range=5.0):
        self.rows, self.cols, self.model = int(rows), int(cols), int(model)
        self.fx, self.fy, self.cx, self.cy, self.range = f64(fx), f64(fy), f64(cx), f64(cy), f64(range)


def _pose(T_cw, cam_pos):
    return np.asarray(T_cw, dtype=f64).reshape(3, 4), np.asarray(cam_pos, dtype=f64).reshape(3)


def _trunc(v):
    """C++'s float -> int conversion of a value known to be in range"""
    return int(v)


# ---- the literal loops -------------------------------------------------------------------------------------------------
def literal_host(cam, cloud, T_cw, cam_pos):
    """depth_render_node.cpp:112-161 -> the CV_32FC1 image"""
    T, pos = _pose(T_cw, cam_pos)
    width, height = cam.cols, cam.rows
    depth_mat = np.zeros((height, width), dtype=f32)                                     # :117
    with np.errstate(all="ignore"):
        for pt in np.asarray(cloud, dtype=f32).reshape(-1, 3):                           # :126
            if not np.isfinite(pt).all():
                continue                                                                 # deviation 2
            pw = [f64(pt[0]), f64(pt[1]), f64(pt[2])]                                    # :127
            d = [pos[i] - pw[i] for i in range(3)]
            if np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > cam.range:           # :128
                continue
            pc = [((T[i, 0] * pw[0] + T[i, 1] * pw[1]) + T[i, 2] * pw[2]) + T[i, 3] for i in range(3)]  # :130
            if np.isnan(pc[2]):
                continue                                                                 # deviation 2
            if pc[2] <= 0.0:                                                             # :132
                continue
            projected_x = f32(pc[0] / pc[2] * cam.fx + cam.cx)                           # :137
            projected_y = f32(pc[1] / pc[2] * cam.fy + cam.cy)                           # :138
            if np.isnan(projected_x) or np.isnan(projected_y):
                continue                                                                 # deviation 2
            if projected_x < f32(0) or projected_x >= f32(width) or projected_y < f32(0) or projected_y >= f32(height):
                continue                                                                 # :139
            dist = f32(pc[2])                                                            # :143
            r = _trunc(f64(0.0573) * cam.fx / f64(dist) + f64(0.5))                      # :144
            rf = f32(r)
            min_x = max(_trunc(projected_x - rf), 0)                                     # :146
            max_x = min(_trunc(projected_x + rf), width - 1)                             # :147
            min_y = max(_trunc(projected_y - rf), 0)                                     # :148
            max_y = min(_trunc(projected_y + rf), height - 1)                            # :149
            win = depth_mat[min_y:max_y + 1, min_x:max_x + 1]                            # :151-160, every pixel by the
            win[...] = np.where(win.astype(f64) < 1e-3, dist, np.minimum(win, dist))     # same rule (:155-159)
    return depth_mat


def literal_cuda(cam, cloud, T_cw, cam_pos):
    """depth_render.cu:2-56 and pcl_render_node.cpp:300-310 -> the published CV_32FC1 image"""
    T, _ = _pose(T_cw, cam_pos)
    Tf = T.astype(f32)                                                                   # Parameter's float r, t
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)                  # set_para's float arguments
    width, height = cam.cols, cam.rows
    depth = np.full((height, width), 999999, dtype=np.int64)                             # depth_initial :55
    with np.errstate(all="ignore"):
        for pt in np.asarray(cloud, dtype=f32).reshape(-1, 3):
            if not np.isfinite(pt).all():
                continue                                                                 # deviation 2
            x, y, z = pt[0], pt[1], pt[2]
            tp = [((x * Tf[i, 0] + y * Tf[i, 1]) + z * Tf[i, 2]) + Tf[i, 3] for i in range(3)]  # :12-14
            if np.isnan(tp[2]):
                continue                                                                 # deviation 2
            if tp[2] <= f32(0.0):                                                        # :16
                continue
            ud = f64(tp[0] / tp[2] * fx + cx) + f64(0.5)                                 # :21
            vd = f64(tp[1] / tp[2] * fy + cy) + f64(0.5)                                 # :22
            if not (-TWO31 - 1.0 < ud < TWO31 and -TWO31 - 1.0 < vd < TWO31):
                continue                                                                 # deviation 2
            u, v = _trunc(ud), _trunc(vd)
            if u < 0 or u >= width or v < 0 or v >= height:                              # :23
                continue
            dist = tp[2]                                                                 # :27
            mf = dist * f32(1000.0) + f32(0.5)                                           # :28
            if not mf < f32(TWO31):
                continue                                                                 # deviation 2
            dist_mm = _trunc(mf)
            r = _trunc(f64(0.0573) * f64(fx) / f64(dist) + f64(f32(0.5)))                # :32
            y0, y1 = max(v - r, 0), min(v + r, height - 1)                               # :33-39
            x0, x1 = max(u - r, 0), min(u + r, width - 1)
            win = depth[y0:y1 + 1, x0:x1 + 1]
            np.minimum(win, dist_mm, out=win)                                            # :41
    d = depth.astype(f32) / f32(1000.0)                                                  # pcl_render_node.cpp:306
    return np.where(d < f32(500.0), d, f32(0)).astype(f32)                               # :307


def literal(cam, cloud, T_cw, cam_pos):
    return (literal_host if cam.model == HOST_NODE else literal_cuda)(cam, cloud, T_cw, cam_pos)


# ---- the vectorised form -------------------------------------------------------------------------------------------------
def project(cam, cloud, T_cw, cam_pos):
    """every point's fate: dict of arrays over the cloud -- why (KEPT, a cull, an UNDEF_*), px, py (HOST_NODE: the float
    projections; CUDA_NODE: u, v as float64), r, x0, x1, y0, y1 (the clipped window), key (uint32), size (its larger
    side).  Entries of points that are not KEPT are meaningless."""
    T, pos = _pose(T_cw, cam_pos)
    P = np.asarray(cloud, dtype=f32).reshape(-1, 3)
    n = len(P)
    why = np.full(n, -1, dtype=np.int64)

    def settle(mask, code):
        why[(why < 0) & mask] = code

    with np.errstate(all="ignore"):
        settle(~np.isfinite(P).all(axis=1), UNDEF_NONFINITE)
        if cam.model == HOST_NODE:
            x, y, z = (P[:, i].astype(f64) for i in range(3))
            dx, dy, dz = pos[0] - x, pos[1] - y, pos[2] - z
            settle(np.sqrt((dx * dx + dy * dy) + dz * dz) > cam.range, RANGE)
            pc = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
            settle(np.isnan(pc[2]), UNDEF_NONFINITE)
            settle(pc[2] <= 0.0, BEHIND)
            px = (pc[0] / pc[2] * cam.fx + cam.cx).astype(f32)
            py = (pc[1] / pc[2] * cam.fy + cam.cy).astype(f32)
            settle(np.isnan(px) | np.isnan(py), UNDEF_NONFINITE)
            settle((px < f32(0)) | (px >= f32(cam.cols)) | (py < f32(0)) | (py >= f32(cam.rows)), OFFIMG)
            dist = pc[2].astype(f32)
            settle(dist < f32(1e-3), UNDEF_NEAR)
            ok = why < 0
            dist_ok = np.where(ok, dist, f32(1.0))
            r = np.trunc(f64(0.0573) * cam.fx / dist_ok.astype(f64) + f64(0.5)).astype(np.int64)
            rf = r.astype(f32)
            pxo, pyo = np.where(ok, px, f32(0)), np.where(ok, py, f32(0))
            hx, hy = pxo + rf, pyo + rf
            x0 = np.maximum(np.trunc(pxo - rf).astype(np.int64), 0)
            y0 = np.maximum(np.trunc(pyo - rf).astype(np.int64), 0)
            x1 = np.where(hx >= f32(TWO31), cam.cols - 1, np.minimum(np.trunc(np.minimum(hx, f32(1e9))).astype(np.int64), cam.cols - 1))
            y1 = np.where(hy >= f32(TWO31), cam.rows - 1, np.minimum(np.trunc(np.minimum(hy, f32(1e9))).astype(np.int64), cam.rows - 1))
            key = dist_ok.view(np.uint32).copy()
            a, b = px.astype(f64), py.astype(f64)
        else:
            Tf = T.astype(f32)
            fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            tp = [((x * Tf[i, 0] + y * Tf[i, 1]) + z * Tf[i, 2]) + Tf[i, 3] for i in range(3)]
            settle(np.isnan(tp[2]), UNDEF_NONFINITE)
            settle(tp[2] <= f32(0.0), BEHIND)
            ud = (tp[0] / tp[2] * fx + cx).astype(f64) + f64(0.5)
            vd = (tp[1] / tp[2] * fy + cy).astype(f64) + f64(0.5)
            settle(~((ud > -TWO31 - 1.0) & (ud < TWO31) & (vd > -TWO31 - 1.0) & (vd < TWO31)), UNDEF_INT)
            live = why < 0
            u = np.trunc(np.where(live, ud, 0.0)).astype(np.int64)
            v = np.trunc(np.where(live, vd, 0.0)).astype(np.int64)
            settle((u < 0) | (u >= cam.cols) | (v < 0) | (v >= cam.rows), OFFIMG)
            settle(tp[2] < f32(1e-3), UNDEF_NEAR)
            mf = tp[2] * f32(1000.0) + f32(0.5)
            settle(~(mf < f32(TWO31)), UNDEF_INT)
            ok = why < 0
            dist_ok = np.where(ok, tp[2], f32(1.0))
            mm = np.trunc(np.where(ok, mf, f32(0))).astype(np.int64)
            r = np.trunc(f64(0.0573) * f64(fx) / dist_ok.astype(f64) + f64(f32(0.5))).astype(np.int64)
            x0, x1 = np.maximum(u - r, 0), np.minimum(u + r, cam.cols - 1)
            y0, y1 = np.maximum(v - r, 0), np.minimum(v + r, cam.rows - 1)
            key = mm.astype(np.uint32)
            a, b = u.astype(f64), v.astype(f64)
    why[why < 0] = KEPT
    size = np.maximum(x1 - x0, y1 - y0) + 1
    return dict(why=why, px=a, py=b, r=r, x0=x0, x1=x1, y0=y0, y1=y1, key=key, size=size)


def keys_to_metres(cam, keys):
    if cam.model == HOST_NODE:
        return np.where(keys == EMPTY, np.uint32(0), keys).astype(np.uint32).view(f32)
    d = np.minimum(keys, np.uint32(999999)).astype(f32) / f32(1000.0)
    return np.where(d < f32(500.0), d, f32(0)).astype(f32)


def raw_from_metres(metres, k):
    """MapROS::depthPoseCallback's convertTo(CV_16UC1, k) (map_ros.cpp:132-133): OpenCV's 32F -> 16U with a scale is
    saturate_cast<ushort>(cvRound(v * (float)k)), cvRound = round half to even"""
    with np.errstate(all="ignore"):
        v = np.rint(np.asarray(metres, dtype=f32) * f32(k))
    return np.where(v >= f32(65535.0), 65535, np.where(v > f32(0), v, 0)).astype(np.uint16)


def render(cam, cloud, T_cw, cam_pos, k=1000.0, detail=None):
    """-> (metres [rows, cols] f32, raw [rows, cols] u16, stats [4] int32); detail: project()'s result, if at hand"""
    d = detail if detail is not None else project(cam, cloud, T_cw, cam_pos)
    keys = np.full((cam.rows, cam.cols), EMPTY, dtype=np.uint32)
    for i in np.flatnonzero(d["why"] == KEPT):
        win = keys[d["y0"][i]:d["y1"][i] + 1, d["x0"][i]:d["x1"][i] + 1]
        np.minimum(win, d["key"][i], out=win)
    metres = keys_to_metres(cam, keys)
    stats = np.array([(d["why"] == KEPT).sum(), np.isin(d["why"], UNDEF).sum(), (metres != 0).sum(), 0], dtype=np.int32)
    return metres, raw_from_metres(metres, k), stats
