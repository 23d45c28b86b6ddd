"""NumPy restatement of the re-identification's two kernels (include/ppn.h: ppn_people_descr, ppn_reid_update), test
infrastructure only.  Plain loops, all integer: `people_descr` reads the four pixel formats with pitched planes, `reid_update`
applies the gallery's rules 1 to 5 on packed arrays."""
import numpy as np

ROWS, COLS, BANDS, BINS, LEN = 96, 32, 3, 8, 72
SLOTS, SIM_MAX, SLOT_OVERFLOW = 128, 9216, 1
ROI_OK = 0
ALIGN = {"nv12": (2, 2), "i420": (2, 2), "yuyv": (1, 2), "bgr": (1, 1)}


# ---- the surface --------------------------------------------------------------------------------------------------------
def layout(fmt, h, w, pitch=None):
    """(nbytes, pitch, pitch_c, u_offset, v_offset) of one contiguous frame, as rt.yuv_frame_layout and, for "bgr", a packed
    frame of [h][pitch] bytes."""
    row = {"nv12": w, "i420": w, "yuyv": 2 * w, "bgr": 3 * w}[fmt]
    pitch = row if pitch is None else pitch
    assert pitch >= row
    if fmt in ("yuyv", "bgr"):
        return h * pitch, pitch, 0, None, None
    if fmt == "nv12":
        return h * pitch + (h // 2) * pitch, pitch, pitch, h * pitch, None
    pc = pitch // 2
    return h * pitch + 2 * (h // 2) * pc, pitch, pc, h * pitch, h * pitch + (h // 2) * pc


def pixel(frame, fmt, h, w, y, x, pitch=None):
    """(c0, c1, c2) of source pixel (y, x) of one frame's bytes: (Y, U, V), for "bgr" (G, B, R)."""
    _, pitch, pc, uo, vo = layout(fmt, h, w, pitch)
    if fmt == "bgr":
        p = y * pitch + 3 * x
        return int(frame[p + 1]), int(frame[p]), int(frame[p + 2])
    if fmt == "yuyv":
        row = y * pitch
        return int(frame[row + 2 * x]), int(frame[row + 4 * (x >> 1) + 1]), int(frame[row + 4 * (x >> 1) + 3])
    c0 = int(frame[y * pitch + x])
    if fmt == "nv12":
        c = uo + (y >> 1) * pc + 2 * (x >> 1)
        return c0, int(frame[c]), int(frame[c + 1])
    c = (y >> 1) * pc + (x >> 1)
    return c0, int(frame[uo + c]), int(frame[vo + c])


def bins(fmt, c):
    """The three bins of a pixel's channels."""
    wide = lambda v: v >> 5
    mid = lambda v: (min(max(v, 64), 191) - 64) >> 4
    return (wide(c[0]), wide(c[1]), wide(c[2])) if fmt == "bgr" else (wide(c[0]), mid(c[1]), mid(c[2]))


def good(rect, status, fmt, h, w):
    y0, x0, rh, rw = (int(v) for v in rect)
    if int(status) != ROI_OK or y0 < 0 or x0 < 0 or rh < 1 or rw < 1 or y0 + rh > h or x0 + rw > w:
        return False
    ay, ax = ALIGN[fmt]
    return not (y0 % ay or rh % ay or x0 % ax or rw % ax)


def describe(frame, fmt, h, w, rect, pitch=None):
    """u16 [72] of one good rectangle."""
    y0, x0, rh, rw = (int(v) for v in rect)
    d = np.zeros((BANDS, 3, BINS), np.int64)
    for i in range(ROWS):
        y = y0 + ((2 * i + 1) * rh) // (2 * ROWS)
        for j in range(COLS):
            x = x0 + ((2 * j + 1) * rw) // (2 * COLS)
            for ch, q in enumerate(bins(fmt, pixel(frame, fmt, h, w, y, x, pitch))):
                d[i // 32, ch, q] += 1
    return d.reshape(LEN).astype(np.uint16)


def people_descr(raw, fmt, h, w, roi, status, pitch=None):
    """raw u8 [F, >= frame bytes], roi i32 [F, R, 4], status i32 [F, R] -> (descr u16 [F, R, 72], valid i32 [F, R])."""
    roi, status = np.asarray(roi), np.asarray(status)
    Fr, R = status.shape
    descr, valid = np.zeros((Fr, R, LEN), np.uint16), np.zeros((Fr, R), np.int32)
    for f in range(Fr):
        for r in range(R):
            if good(roi[f, r], status[f, r], fmt, h, w):
                descr[f, r], valid[f, r] = describe(raw[f], fmt, h, w, roi[f, r], pitch), 1
    return descr, valid


def similarity(a, b):
    return int(np.minimum(np.asarray(a, np.int64), np.asarray(b, np.int64)).sum())


# ---- the gallery --------------------------------------------------------------------------------------------------------
def make_cfg(thr=6452, min_lost=1, memory=300, shift=2, max_rois=64):
    return dict(thr=thr, min_lost=min_lost, memory=memory, shift=shift, max_rois=max_rois)


def fresh_state(streams):
    """All zero bytes: a fresh gallery."""
    z = lambda *s: np.zeros(s, np.int32)
    return dict(pid=z(streams, SLOTS), tid=z(streams, SLOTS), lost=z(streams, SLOTS), n=z(streams, SLOTS),
                descr=np.zeros((streams, SLOTS, LEN), np.uint16), last_pid=z(streams), flags=z(streams))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def fresh_outputs(B, M):
    return dict(pid=np.full((B, M), -1, np.int32), sim=np.full((B, M), -1, np.int32), live=np.full(B, -1, np.int32))


def assert_invariant(st, cfg=None):
    for s in range(st["pid"].shape[0]):
        live = st["pid"][s] != 0
        tids = st["tid"][s][live]
        assert (tids > 0).all() and len(set(tids.tolist())) == len(tids), "live entries hold distinct positive tids"
        pids = st["pid"][s][live]
        assert (pids > 0).all() and len(set(pids.tolist())) == len(pids) and (pids <= st["last_pid"][s]).all()
        for n in ("tid", "lost", "n"):
            assert not st[n][s][~live].any(), f"a free entry has a non-zero {n}"
        assert (st["lost"][s] >= 0).all() and (st["n"][s] >= 0).all() and (st["n"][s] <= 65535).all()
        if cfg is not None:
            assert (st["lost"][s] <= cfg["memory"]).all()


def _take(st, s, e, d, shift):
    if st["n"][s, e] == 0:
        st["descr"][s, e] = d
    else:
        old = st["descr"][s, e].astype(np.int64)
        st["descr"][s, e] = ((old * ((1 << shift) - 1) + d.astype(np.int64) + ((1 << shift) >> 1)) >> shift).astype(np.uint16)
    st["n"][s, e] = min(int(st["n"][s, e]) + 1, 65535)


def reid_update(cfg, st, count, ids, descr, valid, streams, frames, n_frames=None, out=None):
    """One call.  count i32 [B], ids i32 [B, M], descr u16 [B, R, 72], valid i32 [B, R] with B = streams * frames and
    R = cfg["max_rois"]; `st` is updated in place; `out` (fresh_outputs, or arrays filled with a sentinel) is written as the
    kernel writes it."""
    B, M = ids.shape
    R = cfg["max_rois"]
    assert B == streams * frames and descr.shape == (B, R, LEN) and valid.shape == (B, R)
    if out is None:
        out = fresh_outputs(B, M)
    thr, min_lost, memory, shift = cfg["thr"], cfg["min_lost"], cfg["memory"], cfg["shift"]
    for s in range(streams):
        nT = frames if n_frames is None else min(max(int(n_frames[s]), 0), frames)
        for t in range(nT, frames):
            b = s * frames + t
            out["pid"][b], out["sim"][b], out["live"][b] = -1, -1, -1
        pid, tid, lost, n = (st[k][s] for k in ("pid", "tid", "lost", "n"))
        for t in range(nT):
            b = s * frames + t
            P = min(max(int(count[b]), 0), M)
            out["pid"][b], out["sim"][b] = -1, -1
            part = [p for p in range(P) if ids[b, p] > 0]
            has = lambda p: p < R and valid[b, p] != 0
            touched = np.zeros(SLOTS, bool)
            before = copy_state(st)                                  # every comparison sees the state before the frame
            newcomers = []
            for p in part:                                           # 1 bound
                held = [e for e in range(SLOTS) if before["pid"][s, e] != 0 and before["tid"][s, e] == ids[b, p]]
                if not held:
                    newcomers.append(p)
                    continue
                e = held[0]
                if touched[e]:
                    continue                                         # a repeated id: outside the contract
                touched[e], lost[e] = True, 0
                out["pid"][b, p] = pid[e]
                if has(p):
                    _take(st, s, e, descr[b, p], shift)
            unborn = []
            for p in newcomers:                                      # 2 relink
                best = None
                if has(p):
                    for e in range(SLOTS):
                        if (before["pid"][s, e] != 0 and not touched[e] and before["n"][s, e] > 0
                                and min_lost <= before["lost"][s, e] <= memory):
                            key = (-similarity(before["descr"][s, e], descr[b, p]), int(before["lost"][s, e]), e)
                            if best is None or key < best:
                                best = key
                if best is not None and -best[0] >= thr:
                    e = best[2]
                    touched[e], tid[e], lost[e] = True, ids[b, p], 0
                    _take(st, s, e, descr[b, p], shift)
                    out["pid"][b, p], out["sim"][b, p] = pid[e], -best[0]
                else:
                    unborn.append(p)
            for e in range(SLOTS):                                   # 3 age
                if pid[e] != 0 and not touched[e]:
                    lost[e] += 1
                    if lost[e] > memory:
                        pid[e] = tid[e] = lost[e] = n[e] = 0
            free = [e for e in range(SLOTS) if pid[e] == 0]
            for p in unborn:                                         # 4 births
                if not free:
                    st["flags"][s] |= SLOT_OVERFLOW
                    continue
                e = free.pop(0)
                st["last_pid"][s] += 1
                pid[e], tid[e], lost[e], n[e] = st["last_pid"][s], ids[b, p], 0, 0
                if has(p):
                    _take(st, s, e, descr[b, p], shift)
                out["pid"][b, p] = pid[e]
            out["live"][b] = int((pid != 0).sum())
    return out
