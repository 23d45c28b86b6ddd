"""NumPy restatement of ppn_clip_push and ppn_clip_gather (include/ppn.h) on the packed arrays: plain loops over slots and
people, every f32 step a NumPy f32 scalar operation that is rounded on its own, as the kernels' are.  `clip_push` updates
the state in place and returns out_row; `clip_gather` returns (out, out_id, out_len), so a test compares all of them."""
import numpy as np

F = np.float32
SLOTS, MAX_LEN = 64, 256
NORM_NONE, NORM_ROOT = 0, 1
SLOT_OVERFLOW = 1


def make_cfg(K=18, length=32, max_gap=15, norm=NORM_ROOT):
    return dict(K=K, length=length, max_gap=max_gap, norm=norm)


def fresh_state(streams, K, T):
    """All zero bytes: fresh clips."""
    return dict(id=np.zeros((streams, SLOTS), np.int32), gap=np.zeros((streams, SLOTS), np.int32),
                len=np.zeros((streams, SLOTS), np.int32), ref=np.zeros((streams, SLOTS, 4), F),
                mask=np.zeros((streams, SLOTS, T), np.uint32), ring=np.zeros((streams, SLOTS, T, 3, K), F),
                pos=np.zeros(streams, np.int32), flags=np.zeros(streams, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def person_row(K, kp_cell, bbox, score, xy):
    """(planes f32 [3, K], presence mask) of one person: kp_cell i32[K], bbox f32[K,4], score f32[K], xy f32[K,2] or None."""
    row, mask = np.zeros((3, K), F), 0
    for k in range(K):
        if kp_cell[k] < 0:
            continue
        mask |= 1 << k
        if xy is not None:
            row[0, k], row[1, k] = xy[k, 0], xy[k, 1]
        else:
            box = bbox[k]
            row[0, k] = F(F(box[1]) + F(box[3])) * F(0.5)
            row[1, k] = F(F(box[0]) + F(box[2])) * F(0.5)
        row[2, k] = score[k]
    return row, mask


def clip_push(cfg, st, count, kp_cell, bbox, score, ids, xy, streams, frames, n_frames=None, out_row=None):
    """One call.  count i32[B], kp_cell i32[B,M,K], bbox f32[B,M,K,4], score f32[B,M,K], ids i32[B,M], xy f32[B,M,K,2] or
    None, B = streams * frames; `st` is updated in place; `out_row` (or a fresh array) is written as the kernel writes it."""
    K, T = cfg["K"], cfg["length"]
    B, M = kp_cell.shape[:2]
    assert B == streams * frames and kp_cell.shape[2] == K
    if out_row is None:
        out_row = np.zeros((B, M), np.int32)
    for s in range(streams):
        nT = frames if n_frames is None else min(max(int(n_frames[s]), 0), frames)
        for t in range(nT, frames):
            out_row[s * frames + t] = -1
        sid, sgap, slen, sref, smask, sring = (st[n][s] for n in ("id", "gap", "len", "ref", "mask", "ring"))
        for t in range(nT):
            b = s * frames + t
            P = min(max(int(count[b]), 0), M)
            r = int(st["pos"][s])
            out_row[b] = -1
            part = [p for p in range(P) if ids[b, p] > 0]                      # a
            rows = {p: person_row(K, kp_cell[b, p], bbox[b, p], score[b, p], None if xy is None else xy[b, p]) for p in part}
            holder = {}                                                         # id -> live slot, before the frame
            for i in range(SLOTS):
                if sid[i] != 0:
                    holder.setdefault(int(sid[i]), i)
            seen = {}                                                           # slot -> person
            for p in part:
                i = holder.get(int(ids[b, p]))
                if i is not None:
                    seen.setdefault(i, p)
                    out_row[b, p] = i

            def take(i, p):
                sring[i, r], smask[i, r] = rows[p]
                sref[i] = bbox[b, p, 0]

            for i in range(SLOTS):
                if sid[i] == 0:
                    continue
                if i in seen:                                                   # b
                    take(i, seen[i])
                    sgap[i], slen[i] = 0, min(slen[i] + 1, T)
                else:                                                           # c
                    sring[i, r], smask[i, r] = 0, 0
                    sgap[i] += 1
                    slen[i] = min(slen[i] + 1, T)
                    if sgap[i] > cfg["max_gap"]:
                        sid[i] = sgap[i] = slen[i] = 0
            for p in part:                                                      # d
                if int(ids[b, p]) in holder:
                    continue
                free = [i for i in range(SLOTS) if sid[i] == 0]
                if not free:
                    st["flags"][s] |= SLOT_OVERFLOW
                    continue
                i = free[0]
                sid[i], sgap[i], slen[i] = ids[b, p], 0, 1
                take(i, p)
                out_row[b, p] = i
            st["pos"][s] = (r + 1) % T                                          # e
    return out_row


def clip_gather(cfg, st, streams):
    K, T = cfg["K"], cfg["length"]
    out = np.zeros((streams, SLOTS, 3, T, K), F)
    with np.errstate(all="ignore"):
        for s in range(streams):
            pos = int(st["pos"][s])
            for i in range(SLOTS):
                if st["id"][s, i] == 0:
                    continue
                ref = st["ref"][s, i]
                cx = F(F(ref[1]) + F(ref[3])) * F(0.5)
                cy = F(F(ref[0]) + F(ref[2])) * F(0.5)
                h, w = F(F(ref[2]) - F(ref[0])), F(F(ref[3]) - F(ref[1]))
                sc = h if h > w else w
                if not sc > 0:
                    sc = F(1.0)
                for j in range(max(T - int(st["len"][s, i]), 0), T):
                    row = (pos + j) % T
                    src = st["ring"][s, i, row]
                    if cfg["norm"] == NORM_NONE:
                        out[s, i, :, j] = src
                        continue
                    present = (int(st["mask"][s, i, row]) >> np.arange(K) & 1).astype(bool)
                    out[s, i, 0, j] = np.where(present, (src[0] - cx).astype(F) / sc, F(0))
                    out[s, i, 1, j] = np.where(present, (src[1] - cy).astype(F) / sc, F(0))
                    out[s, i, 2, j] = src[2]
    return out, st["id"][:streams].copy(), st["len"][:streams].copy()
