"""The checked BatchNorm-sum handoff on the device (train.ConvStats generation rule): whichever launch overwrites the BatchNorm
workspace between the launch that folded the sums and the BatchNorm that would take them, the handoff is refused on the host.
Ordinary launches only; the bookkeeping itself is covered without a device in test_train_host_cpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mods():
    from pytorch_pose_proposal_network_amd import train as T
    return T


def _stale_setup():
    T = _mods()
    dev = torch.device("cuda")
    xb = torch.randn(2, 24, 24, 128, device=dev).to(torch.bfloat16)
    w = torch.randn(128, 128, 3, 3, device=dev) * 0.03
    g, b = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    return T, xb, w, g, b


def test_statistics_overwritten_by_another_batchnorm_are_refused():
    """The handoff is checked, not a convention: a BatchNorm of ANOTHER tensor with the same channel count on the same stream
    overwrites the workspace the convolution's sums sit in; the BatchNorm of the convolution's output must then refuse the stale
    ConvStats (a host exception -- three ordinary launches) instead of folding the other tensor's sums."""
    T, xb, w, g, b = _stale_setup()
    out, st = T.conv2d_nhwc(xb, w, 1, 1, 1, stats="fwd")
    assert st.blocks > 0
    T.bn_train_forward(torch.randn_like(out), g, b, act="relu")
    with pytest.raises(ValueError):
        T.bn_train_forward(out, g, b, act="relu", stats=st)
    y0, s0 = T.bn_train_forward(out, g, b, act="relu")                      # without the handoff: the ordinary reduction pass
    out2, st2 = T.conv2d_nhwc(xb, w, 1, 1, 1, stats="fwd")                  # a fresh handoff is taken again
    y1, s1 = T.bn_train_forward(out2, g, b, act="relu", stats=st2)
    torch.testing.assert_close(s1.mean, s0.mean, rtol=1e-5, atol=1e-6)
    torch.cuda.synchronize()


@pytest.mark.parametrize("writer", ["bn_backward", "stats_conv", "colsum"])
def test_every_other_workspace_writer_invalidates_the_statistics(writer):
    T, xb, w, g, b = _stale_setup()
    _, saved = T.bn_train_forward(xb, g, b, act="relu")
    out, st = T.conv2d_nhwc(xb, w, 1, 1, 1, stats="fwd")
    assert st.blocks > 0
    if writer == "bn_backward":
        T.bn_train_backward(xb, torch.randn_like(xb), g, b, saved, act="relu")
    elif writer == "stats_conv":
        T.conv2d_nhwc(xb, w, 1, 1, 1, stats="fwd")
    else:
        T.colsum(torch.randn_like(xb), torch.empty(128, device=xb.device))
    with pytest.raises(ValueError):
        T.bn_train_forward(out, g, b, act="relu", stats=st)
    torch.cuda.synchronize()
