"""NumPy restatement of ppn_track_update (include/ppn.h) on the packed arrays: plain loops over p, i and k, every f32 step a
NumPy f32 scalar operation that is rounded on its own, as the kernel's is.  It updates the state in place and returns the
outputs, so a test compares both.

`fused=True` evaluates the keypoint gate the way a contracting compiler would -- dx * dx + dy * dy as fma(dx, dx, dy * dy),
emulated in float64 -- and is there only so that the knife-edge sweep can show that it tells the two apart."""
import numpy as np

F = np.float32
SLOTS, MAX_DET = 64, 256
DET_OVERFLOW, SLOT_OVERFLOW = 1, 2


def make_cfg(K=18, iou_thr=0.3, kp_gate=0.1, min_close=3, max_age=15, birth_thr=0.0, alpha=1.0):
    return dict(K=K, iou_thr=iou_thr, kp_gate=kp_gate, min_close=min_close, max_age=max_age, birth_thr=birth_thr, alpha=alpha)


def fresh_state(streams, K):
    """All zero bytes: a fresh tracker."""
    return dict(id=np.zeros((streams, SLOTS), np.int32), miss=np.zeros((streams, SLOTS), np.int32),
                hits=np.zeros((streams, SLOTS), np.int32), mask=np.zeros((streams, SLOTS), np.uint32),
                root=np.zeros((streams, SLOTS, 4), F), xy=np.zeros((streams, SLOTS, K, 2), F),
                last_id=np.zeros(streams, np.int32), flags=np.zeros(streams, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def fresh_outputs(B, M, K, want_xy=True):
    return dict(ids=np.full((B, M), -1, np.int32), hits=np.zeros((B, M), np.int32),
                xy=np.zeros((B, M, K, 2), F) if want_xy else None, live=np.full(B, -1, np.int32))


def area(b):
    return F(F(b[2]) - F(b[0])) * F(F(b[3]) - F(b[1]))


def iou(bi, ai, bp, ap):
    tl0, tl1 = max(F(bi[0]), F(bp[0])), max(F(bi[1]), F(bp[1]))
    br0, br1 = min(F(bi[2]), F(bp[2])), min(F(bi[3]), F(bp[3]))
    inter = F(F(br0 - tl0) * F(br1 - tl1)) * (F(1) if (tl0 < br0 and tl1 < br1) else F(0))
    with np.errstate(all="ignore"):
        v = F(inter) / F(F(ai + ap) - inter)
    return F(v) if v > 0 else F(0)


def centre(box):
    return F(F(box[1]) + F(box[3])) * F(0.5), F(F(box[0]) + F(box[2])) * F(0.5)


def gate_distance(px, py, tx, ty, fused=False):
    dx, dy = F(px - tx), F(py - ty)
    yy = F(dy * dy)
    if fused:
        return F(np.float64(dx) * np.float64(dx) + np.float64(yy))
    return F(F(dx * dx) + yy)


def track_update(cfg, st, count, kp_cell, bbox, score, streams, frames, n_frames=None, out=None, want_xy=True, fused=False):
    """One call.  count i32[B], kp_cell i32[B,M,K], bbox f32[B,M,K,4], score f32[B,M,K] with B = streams * frames; `st` is
    updated in place; `out` (fresh_outputs, or arrays a test filled with a sentinel) is written as the kernel writes it."""
    K = cfg["K"]
    B, M = kp_cell.shape[:2]
    assert B == streams * frames and kp_cell.shape[2] == K
    if out is None:
        out = fresh_outputs(B, M, K, want_xy)
    alpha, iou_thr, birth_thr = F(cfg["alpha"]), F(cfg["iou_thr"]), F(cfg["birth_thr"])
    gate2 = F(F(cfg["kp_gate"]) * F(cfg["kp_gate"]))
    for s in range(streams):
        nT = frames if n_frames is None else min(max(int(n_frames[s]), 0), frames)
        for t in range(nT, frames):
            b = s * frames + t
            out["ids"][b], out["hits"][b], out["live"][b] = -1, 0, -1
        sid, smiss, shits, smask, sroot, sxy = (st[n][s] for n in ("id", "miss", "hits", "mask", "root", "xy"))
        for t in range(nT):
            b = s * frames + t
            P = min(max(int(count[b]), 0), M)
            D = min(P, MAX_DET)
            if P > D:
                st["flags"][s] |= DET_OVERFLOW
            pmask = [sum(1 << k for k in range(K) if kp_cell[b, p, k] >= 0) for p in range(P)]
            raw = np.zeros((P, K, 2), F)
            for p in range(P):
                for k in range(K):
                    if pmask[p] >> k & 1:
                        raw[p, k] = centre(bbox[b, p, k])
            # 1, 2: the ordered walk on the state as it was before the frame
            taken = [-1] * SLOTS                                   # slot -> person
            slot_of = [-1] * P
            for p in range(D):
                if not pmask[p] & 1:
                    continue
                ap = area(bbox[b, p, 0])
                best, best_key = -1, None
                for i in range(SLOTS):
                    if sid[i] == 0 or taken[i] >= 0:
                        continue
                    ai = area(sroot[i])
                    v = iou(sroot[i], ai, bbox[b, p, 0], ap)
                    r2 = F(gate2 * ai)
                    n_close = 0
                    for k in range(1, K):
                        if (pmask[p] >> k & 1) and (int(smask[i]) >> k & 1):
                            if gate_distance(raw[p, k, 0], raw[p, k, 1], sxy[i, k, 0], sxy[i, k, 1], fused) <= r2:
                                n_close += 1
                    if not (v >= iou_thr or n_close >= cfg["min_close"]):
                        continue
                    key = (n_close, v)
                    if best_key is None or key > best_key:         # strictly greater: the lowest slot of equal keys
                        best, best_key = i, key
                if best >= 0:
                    taken[best], slot_of[p] = p, best
            # 3, 4
            for i in range(SLOTS):
                if sid[i] == 0:
                    continue
                p = taken[i]
                if p >= 0:
                    sroot[i] = bbox[b, p, 0]
                    for k in range(K):
                        if pmask[p] >> k & 1:
                            for c in range(2):
                                if (int(smask[i]) >> k & 1) and alpha != F(1):
                                    old = F(sxy[i, k, c])
                                    sxy[i, k, c] = F(old + F(alpha * F(raw[p, k, c] - old)))
                                else:
                                    sxy[i, k, c] = raw[p, k, c]
                    smask[i], smiss[i] = pmask[p], 0
                    shits[i] += 1
                else:
                    smiss[i] += 1
                    if smiss[i] > cfg["max_age"]:
                        sid[i], smask[i], shits[i], smiss[i] = 0, 0, 0, 0
            # 5
            for p in range(D):
                if not pmask[p] & 1 or slot_of[p] >= 0 or not F(score[b, p, 0]) >= birth_thr:
                    continue
                free = [i for i in range(SLOTS) if sid[i] == 0]
                if not free:
                    st["flags"][s] |= SLOT_OVERFLOW
                    continue
                i = free[0]
                st["last_id"][s] += 1
                sid[i], shits[i], smiss[i], smask[i] = st["last_id"][s], 1, 0, pmask[p]
                sroot[i] = bbox[b, p, 0]
                for k in range(K):
                    if pmask[p] >> k & 1:
                        sxy[i, k] = raw[p, k]
                slot_of[p] = i
            # 6
            out["ids"][b], out["hits"][b] = -1, 0
            for p in range(P):
                i = slot_of[p]
                if i >= 0:
                    out["ids"][b, p], out["hits"][b, p] = sid[i], shits[i]
                if out["xy"] is not None:
                    for k in range(K):
                        if pmask[p] >> k & 1:
                            out["xy"][b, p, k] = sxy[i, k] if i >= 0 else raw[p, k]
                        else:
                            out["xy"][b, p, k] = 0
            out["live"][b] = int((sid != 0).sum())
    return out
