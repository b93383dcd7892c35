"""KinodynamicAstar::search + getSamples as FastPlannerManager::kinodynamicReplan calls them (path_searching/src/
kinodynamic_astar.cpp:15-263, 543-634; plan_manage/src/planner_manager.cpp:124-164), restated: static mode, the first
search with init = true, after NO_PATH reset() and one retry with init = false.

What is literal: the double loop over inputs and durations with its order-dependent bookkeeping (tmp_expand_nodes
compared by f, open nodes by g, both rewritten in place, the pool running out in the middle), the two heap routines of
libstdc++ (heapq is a different heap: the order of equal and of stale keys differs) run on keys that may have gone
stale, the accumulating loops that build the primitive lists, the shot's accumulated checks, getSamples.  The arithmetic
of one expansion's primitives (stateTransit, the tests, estimateHeuristic) is evaluated for all primitives at once with
numpy: every operation is an IEEE f64 + - * / sqrt in the reference's order, element by element.  Every libm result
(cbrt, acos, cos, pow(., 3)) goes through Search.lm: the plain run calls glibc, a seeded run nudges each result by a
random -4 .. +4 ulp -- the stand-in for another libm (the device's).

count=True adds counters that describe what the DEVICE does for the same sequence and change nothing of the above: a model
of the kernel's open-addressing table (TableModel: displaced inserts, longest probe, wraps, look-ups that pass another
node's slot) and the order-dependent events by the wave of their lane (wave_counts)."""
import ctypes
import math
import struct

import numpy as np

REACH_HORIZON, REACH_END, NO_PATH, NEAR_END, CLOSE_GOAL, OVER = 1, 2, 3, 4, 5, -1
MAX_PRIMS, MAX_SEG = 256, 1 << 20
_libm = ctypes.CDLL("libm.so.6")
_libm.cbrt.restype = ctypes.c_double
_libm.cbrt.argtypes = [ctypes.c_double]

DEFAULTS = dict(max_tau=0.8, init_max_tau=1.0, max_vel=2.25, max_acc=2.0, w_time=10.0, horizon=5.0, resolution=0.1,
                lambda_heu=10.0, res=1 / 2.0, time_res=1 / 1.0, time_res_init=1 / 20.0, ts=0.45 / 2.0, allocate_num=4096,
                check_num=10, optimistic=0, min_seg=8, seg_num=0, max_path_nodes=64, max_samples=256)


class KMap:
    """What the search reads of SDFMap: origin, resolution, size, the exploration box, inflated and unknown voxels."""

    def __init__(self, origin, res, nvox, map_size, box_mind, box_maxd, infl, unk):
        self.origin = np.asarray(origin, dtype=np.float64)
        self.res_inv = 1.0 / float(res)
        self.nvox = np.array(nvox, dtype=np.int64)
        self.map_size = np.asarray(map_size, dtype=np.float64)
        self.box_mind = np.asarray(box_mind, dtype=np.float64)
        self.box_maxd = np.asarray(box_maxd, dtype=np.float64)
        self.infl = np.asarray(infl).reshape(nvox) == 1
        self.unk = np.asarray(unk, dtype=bool).reshape(nvox)

    @classmethod
    def from_device(cls, gm):
        h = gm.syncHost(occupancy=True, inflate=True)
        org = np.array(gm.origin)
        return cls(org, gm.res, gm.nvox, list(gm.cfg.map_size), list(gm.cfg.box_min), list(gm.cfg.box_max), h["inflate"],
                   h["occupancy"] < gm.info.clamp_min_log - 1e-3)

    def in_box(self, pos):
        return np.all((pos > self.box_mind) & (pos < self.box_maxd), axis=-1)

    def _plane(self, plane, pos):
        idx = np.floor((pos - self.origin) * self.res_inv).astype(np.int64)
        inside = np.all((idx >= 0) & (idx < self.nvox), axis=-1)
        out = np.zeros(pos.shape[:-1], dtype=bool)
        i = idx[inside]
        out[inside] = plane[i[:, 0], i[:, 1], i[:, 2]]
        return out

    def inflated(self, pos):  # getInflateOccupancy(pos) == 1 (outside the map: -1)
        return self._plane(self.infl, np.atleast_2d(pos))

    def unknown(self, pos):   # getOccupancy(pos) == UNKNOWN
        return self._plane(self.unk, np.atleast_2d(pos))


def nudge(x, k):
    if k == 0 or x == 0.0 or not math.isfinite(x):
        return x
    i = struct.unpack("<q", struct.pack("<d", abs(x)))[0] + k
    return math.copysign(struct.unpack("<d", struct.pack("<q", i))[0], x)


def _guard(fn, x):
    try:
        return fn(x)
    except (ValueError, OverflowError):
        return math.nan


def primitives(cfg):
    """the two lists of search() (:107-122) with its accumulating loops: (init durations, regular inputs, regular
    durations); None where a list passes MAX_PRIMS"""
    step = cfg["time_res_init"] * cfg["init_max_tau"]
    init, tau = [], step
    while tau <= cfg["init_max_tau"] + 1e-3:
        init.append(tau)
        if len(init) > MAX_PRIMS:
            return None
        tau += step
    acc, a = [], -cfg["max_acc"]
    while a <= cfg["max_acc"] + 1e-3:
        acc.append(a)
        if len(acc) > MAX_PRIMS:
            return None
        a += cfg["max_acc"] * cfg["res"]
    dur, tau = [], cfg["time_res"] * cfg["max_tau"]
    while tau <= cfg["max_tau"]:
        dur.append(tau)
        if len(dur) > MAX_PRIMS:
            return None
        tau += cfg["time_res"] * cfg["max_tau"]
    if len(acc) ** 3 * len(dur) > MAX_PRIMS:
        return None
    inputs = [(ax, ay, az) for ax in acc for ay in acc for az in acc]
    return init, inputs, dur


def heap_push(heap, node):
    """std::push_heap after push_back, comparator f1 > f2 (bits/stl_heap.h __push_heap)"""
    heap.append(node)
    hole = len(heap) - 1
    parent = (hole - 1) // 2
    while hole > 0 and heap[parent].f > node.f:
        heap[hole] = heap[parent]
        hole = parent
        parent = (hole - 1) // 2
    heap[hole] = node


def heap_pop(heap):
    """std::pop_heap + pop_back (__pop_heap, __adjust_heap: the hole walks to a leaf, then __push_heap)"""
    if len(heap) > 1:
        last = len(heap) - 1
        value = heap[last]
        heap[last] = heap[0]
        length = last
        hole = child = 0
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if heap[child].f > heap[child - 1].f:
                child -= 1
            heap[hole] = heap[child]
            hole = child
        if (length & 1) == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            heap[hole] = heap[child - 1]
            hole = child - 1
        parent = (hole - 1) // 2
        while hole > 0 and heap[parent].f > value.f:
            heap[hole] = heap[parent]
            hole = parent
            parent = (hole - 1) // 2
        heap[hole] = value
    heap.pop()


class Node:
    __slots__ = ("index", "state", "g", "f", "input", "duration", "parent", "closed", "serial", "lane")


WAVE, LANES = 64, 256


def voxel_hash(key):
    """the device's hash of a voxel triple: 32-bit unsigned arithmetic, so a negative index counts as its two's
    complement"""
    m = 0xFFFFFFFF
    x, y, z = (int(v) & m for v in key)  # (Python integers: the products pass 64 bits)
    return (x * 73856093 & m) ^ (y * 19349663 & m) ^ (z * 83492791 & m)


def table_slots(allocate_num):
    """the smallest power of two that is at least 2 allocate_num and at least 16"""
    cap = 16
    while cap < 2 * allocate_num:
        cap <<= 1
    return cap


class TableModel:
    """What the device's open-addressing table (linear probing, cleared per search) does for the sequence of inserts and
    lookups of one search.  It describes, it decides nothing: the restatement keeps its nodes in a dict."""

    def __init__(self, allocate_num):
        self.cap = table_slots(allocate_num)
        self.slot = {}
        self.c = dict(slots=self.cap, inserts=0, negative=0, displaced=0, longest_probe=0, wraps=0, lookups=0, lookup_wraps=0,
                      found_closed_displaced=0, found_open_displaced=0)

    def insert(self, node):
        h, steps = voxel_hash(node.index) & (self.cap - 1), 0
        while h in self.slot:
            h, steps = (h + 1) & (self.cap - 1), steps + 1
            self.c["wraps"] += h == 0
        self.slot[h] = node
        self.c["inserts"] += 1
        self.c["negative"] += min(node.index) < 0  # a voxel outside the map, below its origin
        self.c["displaced"] += steps > 0
        self.c["longest_probe"] = max(self.c["longest_probe"], steps)

    def lookup(self, key):
        h, passed = voxel_hash(key) & (self.cap - 1), 0
        self.c["lookups"] += 1
        while h in self.slot and passed < self.cap:
            n = self.slot[h]
            if n.index == key:
                if passed:
                    self.c["found_closed_displaced" if n.closed else "found_open_displaced"] += 1
                return n
            h, passed = (h + 1) & (self.cap - 1), passed + 1
            self.c["lookup_wraps"] += h == 0
        return None


def wave_counts():
    """order-dependent events by the wave (lane // 64) of the primitive; sibling_f_cross: those sibling_f events whose
    first lane (the one that created the sibling) lies in an earlier wave"""
    return {k: [0] * (LANES // WAVE) for k in ("sibling_f", "sibling_f_cross", "open_g")}


class Search:
    def __init__(self, km, cfg=None, seed=None, count=False):
        self.km = km
        self.cfg = dict(DEFAULTS)
        self.cfg.update(cfg or {})
        self.rng = None if seed is None else np.random.default_rng(seed)
        self.count = count
        # tables: one dict per search (TableModel.c); waves: the order-dependent events of the init and of the regular
        # expansions by the wave of their lane
        self.counts = dict(sibling_f=0, open_g=0, stale_pop=0, tables=[], waves=dict(init=wave_counts(), reg=wave_counts()))
        self.prims = primitives(self.cfg)
        self.inv_res = 1.0 / self.cfg["resolution"]
        self.tolerance = math.ceil(1 / self.cfg["resolution"])

    # ---- the libm hook
    def lm(self, fn, x):
        y = _guard(fn, float(x))
        if self.rng is not None:
            y = nudge(y, int(self.rng.integers(-4, 5)))
        return y

    def lmv(self, fn, arr):
        return np.array([self.lm(fn, x) for x in arr], dtype=np.float64)

    def pow3(self, t):
        return self.lm(lambda x: math.pow(x, 3.0), t)

    # ---- arithmetic
    @staticmethod
    def transit(s, um, tau):
        """stateTransit (:657-668): s [6], um [n, 3], tau [n] -> [n, 6]"""
        tau = tau[:, None]
        h = 0.5 * (tau * tau)
        return np.concatenate([(s[:3] + tau * s[3:]) + h * um, s[3:] + tau * um], axis=1)

    def pos_to_index(self, p):
        return np.floor((p - self.km.origin) * self.inv_res).astype(np.int64)

    def cubic_front(self, b, c, d):
        a2, a1, a0 = b / 1, c / 1, d / 1
        Q = (3 * a1 - a2 * a2) / 9
        R = (9 * a1 * a2 - 27 * a0 - 2 * a2 * a2 * a2) / 54
        D = Q * Q * Q + R * R
        y = np.empty_like(D)
        pos, zero = D > 0, D == 0
        neg = ~pos & ~zero
        cb = _libm.cbrt
        if pos.any():
            sq = np.sqrt(D[pos])
            S, T = self.lmv(cb, R[pos] + sq), self.lmv(cb, R[pos] - sq)
            # (the reference computes S, then T: the hook is called in that order per element)
            y[pos] = -a2[pos] / 3 + (S + T)
        if zero.any():
            S = self.lmv(cb, R[zero])
            y[zero] = -a2[zero] / 3 + S + S
        if neg.any():
            q = Q[neg]
            theta = self.lmv(math.acos, R[neg] / np.sqrt(-q * q * q))
            y[neg] = 2 * np.sqrt(-q) * self.lmv(math.cos, theta / 3) - a2[neg] / 3
        return y

    def heuristic(self, x1, x2):
        """estimateHeuristic (:296-329) for x1 [n, 6] against x2 [6]: (value, optimal time)"""
        w = self.cfg["w_time"]
        with np.errstate(all="ignore"):
            dp, v0, v1 = x2[:3] - x1[:, :3], x1[:, 3:], x2[3:]

            def dot(a, b):
                return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
            c1 = -36 * dot(dp, dp)
            c2 = 24 * dot(v0 + v1, dp)
            c3 = -4 * ((dot(v0, v0) + dot(v0, v1)) + dot(v1, v1))
            a3 = np.full_like(c1, 0.0 / w)
            a2, a1, a0 = c3 / w, c2 / w, c1 / w
            y1 = self.cubic_front(-a2, a1 * a3 - 4 * a0, 4 * a2 * a0 - a1 * a1 - a3 * a3 * a0)
            r = a3 * a3 / 4 - a2 + y1
            valid = ~(r < 0)
            R = np.sqrt(r)
            k = 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R
            Dn = np.sqrt(0.75 * a3 * a3 - R * R - 2 * a2 + k)
            En = np.sqrt(0.75 * a3 * a3 - R * R - 2 * a2 - k)
            s = 2 * np.sqrt(y1 * y1 - 4 * a0)
            Dz = np.sqrt(0.75 * a3 * a3 - 2 * a2 + s)
            Ez = np.sqrt(0.75 * a3 * a3 - 2 * a2 - s)
            D, E = np.where(R != 0, Dn, Dz), np.where(R != 0, En, Ez)
            t_bar = np.max(np.abs(x1[:, :3] - x2[:3]), axis=1) / (self.cfg["max_vel"] * 0.5)
            cands = [(-a3 / 4 + R / 2 + D / 2, valid & ~np.isnan(D)), (-a3 / 4 + R / 2 - D / 2, valid & ~np.isnan(D)),
                     (-a3 / 4 - R / 2 + E / 2, valid & ~np.isnan(E)), (-a3 / 4 - R / 2 - E / 2, valid & ~np.isnan(E)),
                     (t_bar, np.ones_like(valid))]
            cost = np.full_like(c1, 100000000.0)
            t_d = t_bar.copy()
            for t, m in cands:
                c = -c1 / (3 * t * t * t) - c2 / (2 * t * t) - c3 / t + w * t
                upd = m & ~(t < t_bar) & (c < cost)
                cost = np.where(upd, c, cost)
                t_d = np.where(upd, t, t_d)
        tie_breaker = 1.0 + 1.0 / 10000
        return 1.0 * (1 + tie_breaker) * cost, t_d

    def shot(self, s1, s2, t_d):
        """computeShotTraj (:331-394): coef [3][4] or None"""
        km = self.km
        p0, dp, v0, v1 = s1[:3], s2[:3] - s1[:3], s1[3:], s2[3:]
        dv = v1 - v0
        a = 1.0 / 6.0 * (-12.0 / (t_d * t_d * t_d) * (dp - v0 * t_d) + 6 / (t_d * t_d) * dv)
        b = 0.5 * (6.0 / (t_d * t_d) * (dp - v0 * t_d) - 2 / t_d * dv)
        coef = np.stack([p0, v0, b, a], axis=1)
        t_delta = t_d / 10
        time, checks = t_delta, 0
        while time <= t_d:
            checks += 1
            if checks > 1000:
                return None
            t2, t3 = time * time, self.pow3(time)
            coord = ((coef[:, 0] * 1.0 + coef[:, 1] * time) + coef[:, 2] * t2) + coef[:, 3] * t3
            if np.any((coord < km.origin) | (coord >= km.map_size)):  # (the reference compares with the SIZE)
                return None
            if km.inflated(coord)[0]:
                return None
            time += t_delta
        return coef

    # ---- search() (:15-263)
    def search(self, start_pt, start_v, start_a, end_pt, end_v, init):
        cfg, km = self.cfg, self.km
        alloc = cfg["allocate_num"]
        self.use_node_num, self.iter_num = 0, 0
        self.is_shot, self.coef, self.t_shot, self.path = False, None, 0.0, []
        serial = 0
        cur = Node()
        cur.parent, cur.closed = None, False
        cur.state = np.concatenate([start_pt, start_v])
        cur.index = tuple(self.pos_to_index(start_pt))
        cur.g = 0.0
        cur.input, cur.duration, cur.serial, cur.lane = np.zeros(3), 0.0, 0, 0
        end_state = np.concatenate([end_pt, end_v])
        end_index = self.pos_to_index(end_pt)
        h, _ = self.heuristic(cur.state[None, :], end_state)
        cur.f = cfg["lambda_heu"] * float(h[0])
        heap = []
        heap_push(heap, cur)
        self.use_node_num += 1
        expanded = {cur.index: cur}
        table = None
        if self.count:
            table = TableModel(alloc)
            table.insert(cur)
            self.counts["tables"].append(table.c)
        init_search = init
        init_d, inputs, durs = self.prims
        while heap:
            cur = heap[0]
            if self.count and cur.f > min(n.f for n in heap):
                self.counts["stale_pop"] += 1
            d = cur.state[:3] - start_pt
            reach_horizon = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) >= cfg["horizon"]
            near_end = all(abs(cur.index[k] - end_index[k]) <= self.tolerance for k in range(3))
            if reach_horizon or near_end:
                self.retrieve(cur)
                if near_end:
                    _, t = self.heuristic(cur.state[None, :], end_state)
                    coef = self.shot(cur.state, end_state, float(t[0]))
                    if coef is not None:
                        self.is_shot, self.coef, self.t_shot = True, coef, float(t[0])
            if reach_horizon:
                return REACH_END if self.is_shot else REACH_HORIZON
            if near_end:
                if self.is_shot:
                    return REACH_END
                return NEAR_END if cur.parent is not None else NO_PATH
            heap_pop(heap)
            cur.closed = True
            self.iter_num += 1
            waves = self.counts["waves"]["init" if init_search else "reg"]
            if init_search:
                um = np.repeat(np.asarray(start_a, dtype=np.float64)[None, :], len(init_d), axis=0)
                tau = np.array(init_d)
                init_search = False
            else:
                um = np.repeat(np.array(inputs), len(durs), axis=0)
                tau = np.tile(np.array(durs), len(inputs))
            # the tests that do not depend on the loop's order, for all primitives at once
            pro = self.transit(cur.state, um, tau)
            ok = km.in_box(pro[:, :3])
            pid = self.pos_to_index(pro[:, :3])
            if table is not None:  # the device looks up every primitive that ends inside the box, before anything changes
                for p in np.nonzero(ok)[0]:
                    assert table.lookup(tuple(pid[p])) is expanded.get(tuple(pid[p]))
            ok &= ~np.any(np.abs(pro[:, 3:]) > cfg["max_vel"], axis=1)
            ok &= ~np.all(pid == np.array(cur.index), axis=1)
            for k in range(1, cfg["check_num"] + 1):
                dt = tau * float(k) / float(cfg["check_num"])
                pos = self.transit(cur.state, um, dt)[:, :3]
                bad = km.inflated(pos) | ~km.in_box(pos)
                if not cfg["optimistic"]:
                    bad |= km.unknown(pos)
                ok &= ~bad
            closed = np.array([(lambda n: n is not None and n.closed)(expanded.get(tuple(i))) for i in pid])
            live = np.nonzero(ok & ~closed)[0]
            g_all = ((um[:, 0] * um[:, 0] + um[:, 1] * um[:, 1] + um[:, 2] * um[:, 2]) + cfg["w_time"]) * tau + cur.g
            f_all = np.zeros(len(tau))
            if len(live):
                hv, _ = self.heuristic(pro[live], end_state)
                f_all[live] = g_all[live] + cfg["lambda_heu"] * hv
            # the loop itself, in its order
            tmp_expand = []
            for p in live:
                key = tuple(pid[p])
                pro_node = expanded.get(key)
                tmp_g, tmp_f = float(g_all[p]), float(f_all[p])
                prune = False
                for e in tmp_expand:
                    if e.index == key:
                        prune = True
                        if tmp_f < e.f:
                            e.f, e.g, e.state, e.input, e.duration = tmp_f, tmp_g, pro[p].copy(), um[p].copy(), float(tau[p])
                            self.counts["sibling_f"] += 1
                            waves["sibling_f"][p // WAVE] += 1
                            waves["sibling_f_cross"][p // WAVE] += e.lane // WAVE < p // WAVE
                        break
                if prune:
                    continue
                if pro_node is None:
                    n = Node()
                    n.index, n.state, n.f, n.g = key, pro[p].copy(), tmp_f, tmp_g
                    n.input, n.duration, n.parent, n.closed = um[p].copy(), float(tau[p]), cur, False
                    serial += 1
                    n.serial, n.lane = serial, int(p)
                    if table is not None:
                        table.insert(n)
                    heap_push(heap, n)
                    expanded[key] = n
                    tmp_expand.append(n)
                    self.use_node_num += 1
                    if self.use_node_num == alloc:
                        return NO_PATH
                elif not pro_node.closed:
                    if tmp_g < pro_node.g:
                        pro_node.state, pro_node.f, pro_node.g = pro[p].copy(), tmp_f, tmp_g
                        pro_node.input, pro_node.duration, pro_node.parent = um[p].copy(), float(tau[p]), cur
                        self.counts["open_g"] += 1
                        waves["open_g"][p // WAVE] += 1
        return NO_PATH

    def retrieve(self, end_node):
        path = [end_node]
        while path[-1].parent is not None:
            path.append(path[-1].parent)
        self.path = path[::-1]

    # ---- getSamples (:543-634)
    def get_samples(self, start_vel):
        cfg = self.cfg
        ts = cfg["ts"]
        T_sum = 0.0
        if self.is_shot:
            T_sum += self.t_shot
        back = self.path[-1]
        node = back
        while node.parent is not None:
            T_sum += node.duration
            node = node.parent
        if self.is_shot:
            t = self.t_shot
            end_vel = self.end_vel.copy()
            end_acc = 2 * self.coef[:, 2] + 6 * self.coef[:, 3] * self.t_shot
        else:
            t = back.duration
            end_vel = node.state[3:].copy()  # the START node's velocity: `node` has walked back to it
            end_acc = back.input.copy()
        if cfg["seg_num"] > 0:
            seg_num = cfg["seg_num"]
        else:
            seg_num = max(cfg["min_seg"], int(min(math.floor(T_sum / ts), MAX_SEG)))
        ts = T_sum / float(seg_num)
        sample_shot = self.is_shot
        node = back
        pts = []
        ti = T_sum
        while ti > -1e-5 and len(pts) < MAX_SEG + 2:
            if sample_shot:
                t2, t3 = t * t, self.pow3(t)
                c = self.coef
                pts.append(((c[:, 0] * 1.0 + c[:, 1] * t) + c[:, 2] * t2) + c[:, 3] * t3)
                t -= ts
                if t < -1e-5:
                    sample_shot = False
                    if node.parent is not None:
                        t += node.duration
            else:
                if node.parent is None:
                    break
                xt = self.transit(node.parent.state, node.input[None, :], np.array([t]))[0]
                pts.append(xt[:3].copy())
                t -= ts
                if t < -1e-5 and node.parent.parent is not None:
                    node = node.parent
                    t += node.duration
            ti -= ts
        pts.reverse()
        start_acc = 2 * self.coef[:, 2] if back.parent is None else node.input.copy()
        derivs = np.stack([np.asarray(start_vel, dtype=np.float64), end_vel, start_acc, end_acc])
        return T_sum, ts, seg_num, np.array(pts).reshape(-1, 3), derivs


def solve(km, prob, cfg=None, seed=None, count=False):
    """kinodynamicReplan up to getSamples for one problem dict(start, vel, acc, goal, goal_vel)"""
    S = Search(km, cfg, seed, count)
    c = S.cfg
    sp, sv, sa, gp, gv = (np.asarray(prob[k], dtype=np.float64) for k in ("start", "vel", "acc", "goal", "goal_vel"))
    out = dict(status=NO_PATH, which=0, iter_num=0, use_node_num=0, n_nodes=0, shot=0, t_shot=0.0, coef=np.zeros((3, 4)),
               T_sum=0.0, ts=0.0, seg_num=0, n_samples=0, samples=np.zeros((0, 3)), derivs=np.zeros((4, 3)), nodes=[],
               counts=S.counts)
    d = sp - gp
    if math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < 1e-2:
        out["status"] = CLOSE_GOAL
        return out
    S.end_vel = gv
    status = S.search(sp, sv, sa, gp, gv, True)
    if status == NO_PATH:
        out["which"] = 1
        status = S.search(sp, sv, sa, gp, gv, False)
    out.update(status=status, iter_num=S.iter_num, use_node_num=S.use_node_num)
    if status == NO_PATH:
        return out
    T_sum, ts, seg_num, pts, derivs = S.get_samples(sv)
    out.update(n_nodes=len(S.path), shot=int(S.is_shot), t_shot=S.t_shot if S.is_shot else 0.0,
               coef=S.coef.copy() if S.is_shot else np.zeros((3, 4)), T_sum=T_sum, ts=ts, seg_num=seg_num,
               n_samples=len(pts), samples=pts, derivs=derivs,
               nodes=[dict(state=n.state.copy(), input=n.input.copy(), duration=n.duration, index=n.index) for n in S.path])
    if len(S.path) > c["max_path_nodes"] or len(pts) > c["max_samples"]:
        out["status"] = OVER
    return out


# ---- robustness against another libm -------------------------------------------------------------------------------
def discrete(r):
    """the outputs a flipped comparison would change"""
    return (r["status"], r["which"], r["iter_num"], r["use_node_num"], r["shot"], r["seg_num"], r["n_samples"],
            tuple(n["index"] for n in r["nodes"]), tuple(tuple(n["input"]) for n in r["nodes"]),
            tuple(n["duration"] for n in r["nodes"]))


CONTINUOUS = ("t_shot", "coef", "T_sum", "ts", "samples", "derivs")
SEEDS = tuple(range(101, 109))


def disagreement(a, b):
    out = {}
    for k in CONTINUOUS:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        out[k] = float(np.abs(x - y).max()) if x.size and x.shape == y.shape else (0.0 if x.shape == y.shape else math.inf)
    return out


_memo = {}


def robustness(km, prob, cfg=None, key=None):
    """(plain result, robust?, largest plain-versus-nudged disagreement per continuous output)"""
    if key is not None and key in _memo:
        return _memo[key]
    plain = solve(km, prob, cfg)
    worst = {k: 0.0 for k in CONTINUOUS}
    robust = True
    for seed in SEEDS:
        r = solve(km, prob, cfg, seed=seed)
        if discrete(r) != discrete(plain):
            robust = False
            continue
        for k, v in disagreement(plain, r).items():
            worst[k] = max(worst[k], v)
    res = (plain, robust, worst)
    if key is not None:
        _memo[key] = res
    return res


def tolerance(worst):
    """what the device may differ by: 100 x the measured disagreement of each continuous output"""
    return {k: 100.0 * v for k, v in worst.items()}


# ---- scenes --------------------------------------------------------------------------------------------------------
MAP_SIZE = (8.0, 8.0, 3.0)
BOX = ((-3.8, -3.8, -0.8), (3.8, 3.8, 1.8))
MAP_RES, GROUND, INFL_STEP = 0.1, -1.0, 2
L_FREE, L_OCC, L_UNKNOWN = math.log(0.12 / 0.88), math.log(0.9 / 0.1), math.log(0.12 / 0.88) - 0.01


def occupancy(blocks=(), unknown=()):
    """log-odds of an 80 x 80 x 30 map: free, with occupied / unknown index blocks ((x0, x1), (y0, y1), (z0, z1))"""
    occ = np.full((80, 80, 30), L_FREE)
    for (x0, x1), (y0, y1), (z0, z1) in unknown:
        occ[x0:x1, y0:y1, z0:z1] = L_UNKNOWN
    for (x0, x1), (y0, y1), (z0, z1) in blocks:
        occ[x0:x1, y0:y1, z0:z1] = L_OCC
    return occ


def host_map(occ):
    """the map the device derives from an occupancy array: cube inflation by INFL_STEP voxels (obstacles stay three
    voxels clear of the map's faces, where the reference's linear-address stamp would wrap)"""
    hit = occ > math.log(0.8 / 0.2)
    infl = np.zeros_like(hit)
    s = INFL_STEP
    for x, y, z in zip(*np.nonzero(hit)):
        infl[max(x - s, 0):x + s + 1, max(y - s, 0):y + s + 1, max(z - s, 0):z + s + 1] = True
    org = (-MAP_SIZE[0] / 2.0, -MAP_SIZE[1] / 2.0, GROUND)
    return KMap(org, MAP_RES, (80, 80, 30), MAP_SIZE, BOX[0], BOX[1], infl.astype(np.int8), occ < L_FREE - 1e-3)


def scene_map(sc):
    km = host_map(occupancy(sc.get("blocks", ()), sc.get("unknown", ())))
    if "box" in sc:
        km.box_mind, km.box_maxd = np.array(sc["box"][0], dtype=np.float64), np.array(sc["box"][1], dtype=np.float64)
    return km


V0, A0, Z0 = (0.3, -0.2, 0.1), (0.1, 0.2, -0.1), (0.0, 0.0, 0.0)


def _prob(goal, start=(-2.0, -1.5, 0.0), vel=V0, acc=A0, goal_vel=Z0):
    return dict(start=start, vel=vel, acc=acc, goal=goal, goal_vel=goal_vel)


def face_value():
    """x of a primitive of the face scenes' init expansion that is the first of the expansion in its voxel (its last
    safety sample is the same point): with the box face ON it, it and every later primitive are outside; one ulp
    further it alone is inside and creates a node"""
    p = _prob((-3.2, -0.7, 0.4))
    tau = np.array(primitives(DEFAULTS)[0])
    pos = Search.transit(np.array(p["start"] + p["vel"]), np.repeat(np.array([p["acc"]]), len(tau), axis=0), tau)
    org = np.array((-MAP_SIZE[0] / 2.0, -MAP_SIZE[1] / 2.0, GROUND))
    vox = np.floor((pos[:, :3] - org) * (1.0 / DEFAULTS["resolution"])).astype(int)
    k = next(k for k in range(8, len(tau)) if not any((vox[k] == vox[j]).all() for j in range(k)))
    return float(pos[k, 0])


def scenes():
    """every scene of tests/test_kino_path_gpu.py: occupied / unknown blocks, the box where it is not BOX, cfg overrides,
    problems ("over": the scene is over max_samples, the call reports the limit).  Every problem has a start velocity and
    a goal offset with three distinct non-zero components."""
    far = (1.1, 0.8, 0.4)
    fx = face_value()
    wall = [((38, 41), (3, 50), (3, 27)), ((38, 41), (58, 77), (3, 27))]
    cell = [((14, 16), (16, 30), (5, 20)), ((24, 26), (16, 30), (5, 20)), ((14, 26), (16, 18), (5, 20)),
            ((14, 26), (28, 30), (5, 20)), ((14, 26), (16, 30), (5, 7)), ((14, 26), (16, 30), (18, 20))]
    out = {
        "open": dict(probs=[_prob(far)]),                                      # init 1 x 20, then 125 x 1; REACH_END by shot
        "near_start": dict(probs=[_prob((-1.5, -1.2, 0.2))]),                  # one-node path, start_acc from the shot
        "pillar_start": dict(blocks=[((22, 25), (24, 30), (3, 27))], probs=[_prob((-1.25, -1.1, 0.2))]),  # NO_PATH twice
        "near_end": dict(blocks=[((45, 47), (25, 70), (3, 27))], probs=[_prob(far)]),
        "horizon": dict(cfg=dict(horizon=2.0), probs=[_prob((2.9, 2.3, 0.6), start=(-3.0, -2.5, 0.0))]),
        "enclosed": dict(blocks=cell, probs=[_prob(far, start=(-2.0, -1.7, 0.25), vel=(0.03, -0.02, 0.01))]),
        "alloc_at": dict(cfg=dict(allocate_num=173), probs=[_prob(far)]),
        "alloc_over": dict(cfg=dict(allocate_num=174), probs=[_prob(far)]),
        "bookkeeping": dict(blocks=wall, probs=[_prob((1.9, 0.8, 0.5))]),
        "unknown_pess": dict(unknown=[((35, 45), (25, 55), (0, 30))], probs=[_prob(far)]),
        "unknown_opt": dict(unknown=[((35, 45), (25, 55), (0, 30))], cfg=dict(optimistic=1), probs=[_prob(far)]),
        "face_on": dict(box=(BOX[0], (fx, BOX[1][1], BOX[1][2])), probs=[_prob((-3.2, -0.7, 0.4))]),
        "face_in": dict(box=(BOX[0], (math.nextafter(fx, math.inf), BOX[1][1], BOX[1][2])), probs=[_prob((-3.2, -0.7, 0.4))]),
        "close_goal": dict(probs=[_prob((-2.0 + 0.008, -1.5 + 0.005, 0.003)), _prob((-2.0 + 0.008, -1.5 + 0.005, 0.0034))]),
        "forced_seg": dict(cfg=dict(seg_num=12), probs=[_prob(far), _prob((-1.5, -1.2, 0.2))]),
    }
    out.update(edge_scenes(out))
    return out


# the wall map's problem the other way round, from the far side back through the gap: the primitives of the last wave
# of a four-wave list (the largest x input) then brake, and land in voxels that are open already
BACK = dict(start=(2.0, -1.5, 0.0), goal=(-1.9, 0.8, 0.5))
# a box that reaches past the map's low x face: a start in it has negative voxel indices
BOX_PAST_MAP = ((-4.6, BOX[0][1], BOX[0][2]), BOX[1])
INIT_LISTS = (1, 63, 64, 65, 255, 256)
# regular lists by their number of primitives: name -> (primitives, cfg); the wall map unless said otherwise
REG_LISTS = {
    "reg1x8": (8, dict(res=2.5, time_res=1 / 8.0)),
    "reg27x2": (54, dict(res=1.0, time_res=1 / 2.0)),
    "reg64": (64, dict(res=2 / 3.0)),
    "reg128": (128, dict(res=2 / 3.0, time_res=1 / 2.0, allocate_num=1024)),
    "reg216": (216, dict(res=0.4)),
    "reg216_back": (216, dict(res=0.4)),
    "reg216_tau": (216, dict(res=0.4, max_tau=0.4, allocate_num=512)),
    "reg250": (250, dict(time_res=1 / 2.0, allocate_num=1024)),
    "reg256": (256, dict(res=2 / 3.0, time_res=1 / 4.0, allocate_num=1024)),
    "reg256_open": (256, dict(res=2 / 3.0, time_res=1 / 4.0)),
}
REG216_NODES = 2029   # use_node_num of reg216
TIGHT = ("tight216", "tight_near_end", "tight16", "tight2", "tight8", "tight9", "retry_short_table")
REFUSED = ("start_out_of_box", "start_out_of_map", "goal_out_of_map", "goal_past_size", "check1")
SAMPLING = tuple("%s_%s" % (k, w) for w in ("shot", "noshot")
                 for k in ("seg1", "seg2", "seg1000_at", "seg1000_over", "minseg_above", "minseg_below", "ts_long"))


def edge_scenes(base):
    """the scenes at the lane, hash and sample-count edges ("What the kinodynamic scenes hold")"""
    far = (1.1, 0.8, 0.4)
    wall, book = base["bookkeeping"]["blocks"], base["bookkeeping"]["probs"][0]
    back = _prob(BACK["goal"], start=BACK["start"])
    fence = base["near_end"]["blocks"]
    sc = {}
    for n in INIT_LISTS:  # the init expansion up to, at and past a wave, and at the workgroup
        sc["init%d" % n] = dict(blocks=wall, cfg=dict(time_res_init=1.0 / n), probs=[dict(book)])
    for name, (_, cfg) in REG_LISTS.items():
        sc[name] = dict(blocks=wall, cfg=dict(cfg), probs=[dict(book)])
    for name in ("reg216_back", "reg216_tau", "reg250", "reg256"):
        sc[name]["probs"] = [dict(back)]
    sc["reg256_open"] = dict(cfg=dict(REG_LISTS["reg256_open"][1]), probs=[_prob(far)])  # three pops: easy to read
    # the pool runs out in the middle of a later, four-wave expansion / one node later it does not
    sc["reg216_at"] = dict(blocks=wall, cfg=dict(res=0.4, allocate_num=REG216_NODES), probs=[dict(book)])
    sc["reg216_over"] = dict(blocks=wall, cfg=dict(res=0.4, allocate_num=REG216_NODES + 1), probs=[dict(book)])
    # tight tables: 4096 slots for 2029 nodes, 512 for 143, 32 and 16 for a pool that runs out in the init expansion
    sc["tight216"] = dict(blocks=wall, cfg=dict(res=0.4, allocate_num=2040), probs=[dict(book)])
    sc["tight_near_end"] = dict(blocks=fence, cfg=dict(allocate_num=200), probs=[_prob(far)])
    for a in (16, 2, 8, 9):
        sc["tight%d" % a] = dict(cfg=dict(allocate_num=a), probs=[_prob(far)])
    # the retry answers, on a table of 128 slots that the first search left with 64 entries: what the workgroup's own
    # clear of fewer slots than lanes left behind would be found
    sc["retry_short_table"] = dict(cfg=dict(res=1.0, allocate_num=64, time_res_init=1 / 64.0),
                                   probs=[_prob((0.1, 2.73, 0.25), start=(2.7, -1.1, 0.3), vel=(0.79, -0.22, 0.12))])
    # starts and goals the search refuses by itself
    sc["start_out_of_box"] = dict(probs=[_prob(far, start=(-3.95, -1.5, 0.0), vel=(-0.3, -0.2, 0.1))])
    sc["start_out_of_map"] = dict(box=BOX_PAST_MAP, probs=[_prob((-1.1, 0.8, 0.4), start=(-4.35, -1.5, 0.0))])
    sc["goal_out_of_map"] = dict(probs=[_prob((-4.3, -0.7, 0.4))])        # below the origin: no shot passes
    sc["goal_past_size"] = dict(probs=[_prob((4.3, 0.8, 0.4))])           # (the reference compares with the SIZE)
    sc["check1"] = dict(blocks=wall, cfg=dict(check_num=1), probs=[dict(book)])
    # getSamples on a multi-node path with the shot and on one without
    for w, blocks, p in (("shot", wall, book), ("noshot", fence, _prob(far))):
        for k, cfg in (("seg1", dict(seg_num=1)), ("seg2", dict(seg_num=2)), ("seg1000_at", dict(seg_num=1000, max_samples=1001)),
                       ("seg1000_over", dict(seg_num=1000, max_samples=1000)), ("minseg_above", dict(min_seg=40)),
                       ("minseg_below", dict(min_seg=5)), ("ts_long", dict(ts=1.0))):
            sc["%s_%s" % (k, w)] = dict(blocks=blocks, cfg=cfg, probs=[dict(p)])
    for name in ("seg1000_over_shot", "seg1000_over_noshot"):
        sc[name]["over"] = True  # status -1: the call reports FUELMI_ELIMIT, the counts are still reported
    return sc


# what the reference holds constant: a scene whose cfg sets one of these has no recorded fixture.  The first four are
# constants of search(), min_seg is the 8 of getSamples.
NOT_IN_REFERENCE = ("res", "time_res", "time_res_init", "seg_num", "min_seg")


def has_fixture(sc):
    return not any(k in sc.get("cfg", {}) for k in NOT_IN_REFERENCE)


def batch65():
    """the open problem first and last, between them seven other problems nine times over: every problem of the batch is
    also a problem the restatement is asked (and checked for robustness), at several block indices"""
    rng = np.random.default_rng(7)
    mid = [_prob(tuple(np.array((1.1, 0.8, 0.4)) + rng.uniform(-0.6, 0.6, 3)),
                 vel=tuple(rng.uniform(0.05, 0.4, 3) * np.array([1, -1, 1]))) for _ in range(7)]
    first = _prob((1.1, 0.8, 0.4))
    return [first] + [dict(mid[i % 7]) for i in range(63)] + [dict(first)]


# one launch with every outcome, on the wall map: ten distinct problems seven times over and the first two once more (72:
# more than one problem per workgroup slot).  max_samples = OUTCOME_CFG's: exactly the problems "back" are over it.
OUTCOME_SCENE, OUTCOME_CFG = "bookkeeping", dict(max_samples=32)


def outcome_problems():
    """(names, the ten problems): REACH_END (four of them, one a one-node path, one over max_samples), NEAR_END,
    REACH_HORIZON twice (a goal past the horizon, a goal outside the map), NO_PATH after the retry twice (a start inside
    the inflation: no primitive survives; a start next to a goal across the wall: the first pop ends the search),
    CLOSE_GOAL (returns before the first barrier)"""
    named = [("book", _prob((1.9, 0.8, 0.5))), ("back", _prob(BACK["goal"], start=BACK["start"])),
             ("behind_wall", _prob((0.5, -1.2, 0.5))), ("horizon_far", _prob((2.9, 2.3, 0.6), start=(-3.0, -2.5, 0.0))),
             ("horizon_out", _prob((4.3, 0.8, 0.4))), ("in_inflation", _prob((1.9, 0.8, 0.5), start=(-0.35, -1.5, 0.0))),
             ("across_wall", _prob((0.5, -1.27, 0.45), start=(-0.5, -1.2, 0.5))),
             ("close", _prob((-2.0 + 0.004, -1.5 + 0.003, 0.002))), ("short", _prob((-1.5, -1.2, 0.2))),
             ("left", _prob((-1.1, 2.8, 0.9)))]
    return [n for n, _ in named], [p for _, p in named]


def outcome_batch():
    names, probs = outcome_problems()
    order = [i % 10 for i in range(72)]
    return [names[i] for i in order], [dict(probs[i]) for i in order]


# the problems of the GPU test's device chain (tests/test_kino_path_gpu.py, load_kino) on the near_end scene's map, with
# seg_num forced to LOAD_SEG: a first load, then a second one whose candidate 1 finds no path (the shot from its start
# crosses the wall, twice) and whose candidate 3 is refused as a close goal
LOAD_SCENE, LOAD_CTRL, LOAD_SEG = "near_end", 14, 11


# (degree, control points) of the other batches the chain is run for: degrees 4 and 5, and the smallest batch of each
# degree, one segment and two samples
LOAD_SIZES = ((4, 15), (5, 16), (3, 4), (4, 5), (5, 6))


def load_problems():
    pa = [_prob(g) for g in ((-0.2, 0.8, 0.4), (-0.5, 1.3, 0.5), (-1.5, 0.9, 0.3), (0.1, -0.6, 0.6))]
    pb = [_prob((-0.4, 1.0, 0.45)), _prob((1.05, 0.9, 0.5), start=(0.1, 0.5, 0.2)), _prob((-0.3, -0.9, 0.35)),
          _prob((-2.0 + 0.004, -1.5 + 0.003, 0.002))]
    return pa, pb


# the MID problem the facade's driver is given (start, viewpoint) on the same map; its goal path is not truncated, so
# the search's goal is the viewpoint
FACADE_SCENE = "near_end"


def facade_problem():
    return _prob((-0.2, 2.3, 0.4))


def problem_results(scene, probs, cfg=None):
    """(plain result, robust, worst disagreement) per problem on a scene's map with cfg on top of the scene's; computed
    once per process and distinct problem"""
    sc = scenes()[scene]
    km = scene_map(sc)
    c = dict(sc.get("cfg", {}))
    c.update(cfg or {})
    out = []
    for p in probs:
        key = (scene, tuple(sorted(c.items())), tuple(tuple(float(v) for v in p[k]) for k in ("start", "vel", "acc", "goal", "goal_vel")))
        out.append(robustness(km, p, c, key=key))
    return out


def scene_results(name, sc=None):
    """(plain result, robust, worst disagreement) per problem of a scene, computed once per process"""
    return problem_results(name, scenes()[name]["probs"])
