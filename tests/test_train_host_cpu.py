"""CPU-only checks of the training host path's bookkeeping (no device, no libppn.so): the generation rule of the BatchNorm-sum
handoff (train.ConvStats / train._Workspace / train._stats_blocks) and the trust test of the limb probe remainder
(train.limb_remainder_trusted)."""
import pytest


class _Tensor:
    """what _stats_blocks reads of a tensor"""

    def __init__(self, ptr):
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr


def test_convstats_is_accepted_at_its_generation_only():
    from pytorch_pose_proposal_network_amd import train as T
    ws, other_ws = T._Workspace(None), T._Workspace(None)
    y, other = _Tensor(0x1000), _Tensor(0x2000)
    ws.written()                                            # the launch that folds the sums (a statistics convolution, say)
    st = T.ConvStats(ws, 7, 1, y)
    assert st.gen == ws.gen == 1
    assert T._stats_blocks(st, ws, 1, y) == 7
    assert T._stats_blocks(st, ws, 1, _Tensor(0x1000)) == 7    # the same memory through another view
    assert T._stats_blocks(None, ws, 1, y) == 0
    for bad in ((ws, 1, other), (ws, 2, y), (other_ws, 1, y)):  # another tensor / pass / workspace
        with pytest.raises(ValueError):
            T._stats_blocks(st, *bad)
    # each of the four writers (bn_train_forward, bn_train_backward, conv2d_nhwc(stats=), colsum) announces its launch
    # with written(): whichever runs in between, the sums are gone
    for _ in range(4):
        st = T.ConvStats(ws, 3, 2, y)
        assert T._stats_blocks(st, ws, 2, y) == 3
        ws.written()
        with pytest.raises(ValueError, match="stale"):
            T._stats_blocks(st, ws, 2, y)
    assert T._stats_blocks(T.ConvStats(ws, 3, 2, y), ws, 2, y) == 3   # the handoff of the newest writer is good again
    other_ws.written()                                      # a workspace of another channel count / stream does not matter
    st = T.ConvStats(ws, 5, 1, y)
    other_ws.written()
    assert T._stats_blocks(st, ws, 1, y) == 5


def test_convstats_without_sums_is_always_accepted():
    """blocks == 0: the launch folded nothing, the BatchNorm runs its own reduction pass -- no check at all"""
    from pytorch_pose_proposal_network_amd import train as T
    ws = T._Workspace(None)
    y = _Tensor(0x1000)
    st = T.ConvStats(ws, 0, 1, y)
    ws.written()
    assert T._stats_blocks(st, ws, 1, y) == 0
    assert T._stats_blocks(st, T._Workspace(None), 2, _Tensor(0x3000)) == 0
    assert T._stats_blocks(T.ConvStats(None, 0, 2, y), ws, 2, y) == 0      # conv_dgrad's parity form: no workspace at all


def test_limb_remainder_trust_thresholds():
    from pytorch_pose_proposal_network_amd import lib as L, train as T
    ok = T.limb_remainder_trusted
    # coeff_4 against 1e-3 of the largest coefficient, either mode
    for dt in (L.PPN_F32, L.PPN_BF16):
        assert ok([1.0, 0.5, 0.2, 0.1, 1.001e-3], dt)
        assert not ok([1.0, 0.5, 0.2, 0.1, 1.0e-3], dt)
        assert not ok([1.0, 0.5, 0.2, 0.1, 0.999e-3], dt)
        assert ok([0.2] * 5, dt)
        assert not ok([0.2, 0.2, 0.2, 0.2, 0.0], dt)
    # ||remainder||^2 against (16 * 2^-8)^2 ||total||^2 = 2^-8 ||total||^2: 16-bit modes only
    thr = 2.0 ** -8
    assert (16.0 * 2.0 ** -8) ** 2 == thr
    assert ok([0.2] * 5, L.PPN_BF16, 1.001 * thr * 3.0, 3.0)
    assert not ok([0.2] * 5, L.PPN_BF16, thr * 3.0, 3.0)
    assert not ok([0.2] * 5, L.PPN_BF16, 0.999 * thr * 3.0, 3.0)
    assert ok([0.2] * 5, L.PPN_F32, 0.999 * thr * 3.0, 3.0) and ok([0.2] * 5, L.PPN_F32, 0.0, 3.0)
    assert not ok([1.0, 0.5, 0.2, 0.1, 1.0e-3], L.PPN_BF16, 3.0, 3.0)       # a large remainder does not rescue a tiny coeff_4
