"""NumPy restatement of ppn_zone_update (include/ppn.h, rules a to g) on the packed arrays: plain loops over people, slots,
zones and lines, every f32 step a NumPy f32 scalar operation that is rounded on its own, as the kernel's is.  `zone_update`
updates the state in place and returns the outputs, so a test compares both."""
import numpy as np

F = np.float32
SLOTS, ZONE_MAX, MAX_VERT, LINE_MAX = 64, 16, 8, 16
ANCHOR_CENTER, ANCHOR_BOTTOM = 0, 1
SLOT_OVERFLOW = 1
I32_MAX = 2 ** 31 - 1


def make_cfg(K=18, max_gap=15, anchor=ANCHOR_CENTER, loiter=1):
    return dict(K=K, max_gap=max_gap, anchor=anchor, loiter=loiter)


def fresh_geom(streams):
    return dict(zone_n=np.zeros(streams, np.int32), zone_nv=np.zeros((streams, ZONE_MAX), np.int32),
                zone_xy=np.zeros((streams, ZONE_MAX, MAX_VERT, 2), F), line_n=np.zeros(streams, np.int32),
                line_xy=np.zeros((streams, LINE_MAX, 4), F))


def make_geom(zones, lines):
    """Per stream a list of polygons [(x, y), ..] and a list of segments (ax, ay, bx, by) -> the tables."""
    g = fresh_geom(len(zones))
    for s, (zs, ls) in enumerate(zip(zones, lines)):
        g["zone_n"][s], g["line_n"][s] = len(zs), len(ls)
        for z, poly in enumerate(zs):
            g["zone_nv"][s, z] = len(poly)
            g["zone_xy"][s, z, :len(poly)] = np.asarray(poly, F).reshape(-1, 2)
        for l, seg in enumerate(ls):
            g["line_xy"][s, l] = seg
    return g


def fresh_state(streams):
    """All zero bytes: fresh."""
    return dict(id=np.zeros((streams, SLOTS), np.int32), gap=np.zeros((streams, SLOTS), np.int32),
                inside=np.zeros((streams, SLOTS), np.uint32), dwell=np.zeros((streams, SLOTS, ZONE_MAX), np.int32),
                last=np.zeros((streams, SLOTS, 2), F), zone_total=np.zeros((streams, ZONE_MAX, 2), np.int32),
                line_total=np.zeros((streams, LINE_MAX, 2), np.int32), flags=np.zeros(streams, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def fresh_outputs(B, M):
    return dict(slot=np.full((B, M), -1, np.int32), inside=np.zeros((B, M), np.uint32),
                zone=np.zeros((B, ZONE_MAX, 4), np.int32), line=np.zeros((B, LINE_MAX, 2), np.int32))


def in_polygon(poly, ax, ay):
    """The even-odd ray test of rule a; poly f32 [nv, 2] of (x, y)."""
    nv, inside = len(poly), False
    for i in range(nv):
        xi, yi = F(poly[i][0]), F(poly[i][1])
        xj, yj = F(poly[i - 1][0]), F(poly[i - 1][1])
        if (yi > ay) != (yj > ay):
            cut = F(F(F(xj - xi) * F(ay - yi)) / F(yj - yi)) + xi
            if ax < F(cut):
                inside = not inside
    return inside


def anchor_of(cfg, box, xy0):
    """(ax, ay) of rule a; box f32[4] = the root box, xy0 the smoothed root centre or None."""
    if xy0 is not None and cfg["anchor"] == ANCHOR_CENTER:
        return F(xy0[0]), F(xy0[1])
    ax = F(F(box[1]) + F(box[3])) * F(0.5)
    ay = F(box[2]) if cfg["anchor"] == ANCHOR_BOTTOM else F(F(box[0]) + F(box[2])) * F(0.5)
    return F(ax), F(ay)


def side(seg, x, y):
    ax, ay, bx, by = (F(v) for v in seg)
    return bool(F(F(F(bx - ax) * F(y - ay)) - F(F(by - ay) * F(x - ax))) >= 0)


def cross(ux, uy, vx, vy):
    return F(F(ux * vy) - F(uy * vx))


def crossing(seg, p0, p1):
    """0: the step p0 -> p1 does not cross the segment, +1: forward, -1: backward (rule c)."""
    s0, s1 = side(seg, *p0), side(seg, *p1)
    if s0 == s1:
        return 0
    ax, ay, bx, by = (F(v) for v in seg)
    ux, uy = F(p1[0] - p0[0]), F(p1[1] - p0[1])
    e0 = cross(ux, uy, F(ax - p0[0]), F(ay - p0[1]))
    e1 = cross(ux, uy, F(bx - p0[0]), F(by - p0[1]))
    if (e0 <= 0 and e1 >= 0) or (e0 >= 0 and e1 <= 0):
        return 1 if s1 else -1
    return 0


def sat_inc(v):
    return min(int(v) + 1, I32_MAX)


def zone_update(cfg, geom, st, count, kp_cell, bbox, ids, xy, streams, frames, n_frames=None, out=None):
    """One call.  count i32[B], kp_cell i32[B,M,K], bbox f32[B,M,K,4], ids i32[B,M], xy f32[B,M,K,2] or None, B = streams *
    frames; `st` is updated in place; `out` (fresh_outputs, or arrays a test filled with a sentinel) is written as the kernel
    writes it."""
    B, M = kp_cell.shape[:2]
    assert B == streams * frames and kp_cell.shape[2] == cfg["K"]
    if out is None:
        out = fresh_outputs(B, M)
    with np.errstate(all="ignore"):
        for s in range(streams):
            nT = frames if n_frames is None else min(max(int(n_frames[s]), 0), frames)
            for t in range(nT, frames):
                b = s * frames + t
                out["slot"][b], out["inside"][b], out["zone"][b], out["line"][b] = -1, 0, 0, 0
            if nT == 0:
                continue
            zone_n = min(max(int(geom["zone_n"][s]), 0), ZONE_MAX)
            line_n = min(max(int(geom["line_n"][s]), 0), LINE_MAX)
            polys = []
            for z in range(zone_n):
                nv = min(max(int(geom["zone_nv"][s, z]), 0), MAX_VERT)
                polys.append(geom["zone_xy"][s, z, :nv] if nv >= 3 else None)
            segs = [geom["line_xy"][s, l] for l in range(line_n)]
            sid, sgap, sin, sdwell, slast = (st[n][s] for n in ("id", "gap", "inside", "dwell", "last"))
            for t in range(nT):
                b = s * frames + t
                P = min(max(int(count[b]), 0), M)
                out["slot"][b], out["inside"][b], out["zone"][b], out["line"][b] = -1, 0, 0, 0
                anchors, in_now, part = {}, {}, []
                for p in range(P):                                                  # a
                    ax, ay = anchor_of(cfg, bbox[b, p, 0], None if xy is None else xy[b, p, 0])
                    valid = kp_cell[b, p, 0] >= 0 and np.isfinite(ax) and np.isfinite(ay)
                    mask = 0
                    if valid:
                        for z, poly in enumerate(polys):
                            if poly is not None and in_polygon(poly, ax, ay):
                                mask |= 1 << z
                    anchors[p], in_now[p] = (ax, ay), mask
                    out["inside"][b, p] = mask
                    for z in range(zone_n):
                        out["zone"][b, z, 0] += mask >> z & 1
                    if valid and ids[b, p] > 0:
                        part.append(p)
                holder = {}                                                         # b: id -> live slot, before the frame
                for i in range(SLOTS):
                    if sid[i] != 0:
                        holder.setdefault(int(sid[i]), i)
                seen = {}                                                           # slot -> person
                for p in part:
                    i = holder.get(int(ids[b, p]))
                    if i is not None:
                        seen.setdefault(i, p)
                        out["slot"][b, p] = i

                def entered(z):
                    out["zone"][b, z, 1] += 1
                    st["zone_total"][s, z, 0] += 1

                def exited(z):
                    out["zone"][b, z, 2] += 1
                    st["zone_total"][s, z, 1] += 1

                for i in range(SLOTS):
                    if sid[i] == 0:
                        continue
                    was = int(sin[i])
                    if i in seen:                                                   # c
                        p = seen[i]
                        p0, p1, now = (F(slast[i, 0]), F(slast[i, 1])), anchors[p], in_now[p]
                        for l, seg in enumerate(segs):
                            d = crossing(seg, p0, p1)
                            if d:
                                out["line"][b, l, 0 if d > 0 else 1] += 1
                                st["line_total"][s, l, 0 if d > 0 else 1] += 1
                        for z in range(zone_n):
                            if now >> z & 1:
                                if was >> z & 1:
                                    sdwell[i, z] = sat_inc(sdwell[i, z])
                                else:
                                    sdwell[i, z] = 1
                                    entered(z)
                            else:
                                sdwell[i, z] = 0
                                if was >> z & 1:
                                    exited(z)
                        sgap[i], sin[i], slast[i] = 0, now, p1
                    else:
                        sgap[i] += 1
                        if sgap[i] > cfg["max_gap"]:                                # f
                            for z in range(zone_n):
                                if was >> z & 1:
                                    exited(z)
                            sid[i] = sgap[i] = sin[i] = 0
                            sdwell[i] = 0
                        else:                                                       # e
                            for z in range(zone_n):
                                if was >> z & 1:
                                    sdwell[i, z] = sat_inc(sdwell[i, z])
                for p in part:                                                      # d
                    if int(ids[b, p]) in holder:
                        continue
                    free = [i for i in range(SLOTS) if sid[i] == 0]
                    if not free:
                        st["flags"][s] |= SLOT_OVERFLOW
                        continue
                    i = free[0]
                    sid[i], sgap[i], sin[i], slast[i] = ids[b, p], 0, in_now[p], anchors[p]
                    for z in range(ZONE_MAX):
                        sdwell[i, z] = in_now[p] >> z & 1
                    for z in range(zone_n):
                        if in_now[p] >> z & 1:
                            entered(z)
                    out["slot"][b, p] = i
                for z in range(zone_n):                                             # g
                    out["zone"][b, z, 3] = sum(1 for i in range(SLOTS) if sid[i] != 0 and sdwell[i, z] >= cfg["loiter"])
    return out


def slots_inside(st, s, z):
    """The live slots of stream s with bit z: what zone_total's entered - exited must equal (rules d and f)."""
    return int(((st["id"][s] != 0) & ((st["inside"][s] >> np.uint32(z) & np.uint32(1)) != 0)).sum())
