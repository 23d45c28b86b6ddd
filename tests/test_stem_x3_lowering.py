"""CPU: how fuse_stem="all" lowers in the exact inference modes (float16x3, float16 with an exact prefix).

The stem becomes ONE split-f16 launch (csrc/stem012_x3.hip, PPN_F16X3 internals, f32 outputs); every launch behind it is the
launch of the mode's default lowering -- same names, dtypes, tensors and fused shortcuts.  The float32 mode keeps rejecting
the fused stem."""
import pytest

from pytorch_pose_proposal_network_amd import lib as L, model


def _sig(net, op):
    return (op.name, net._op_dtype(op), op.src, op.out_raw, op.out_act, op.residual, op.ds_src, op.k, op.stride, op.cin,
            op.cout, op.bn1, op.bn2)


CASES = [("drn_d_22", dict(compute_dtype="float16x3")),
         ("drn_d_38", dict(compute_dtype="float16x3")),
         ("drn_d_54", dict(compute_dtype="float16x3")),
         ("drn_d_22", dict(compute_dtype="float16", exact_prefix=3)),
         ("drn_d_54", dict(compute_dtype="float16", exact_prefix=4))]


@pytest.mark.parametrize("arch,kw", CASES)
def test_fused_x3_stem_lowering(arch, kw):
    base = model.PoseProposalNet(arch, **kw)
    fused = model.PoseProposalNet(arch, fuse_stem="all", **kw)
    stem = fused._ops[0]
    assert stem.k == 7 and stem.next3x3 is not None and stem.next_s2 is not None
    assert fused._op_dtype(stem) == L.PPN_F16X3 and fused._is_x3_stem(stem)
    assert not any(base._is_x3_stem(o) for o in base._ops)
    # the default lowering runs the same three layers as three exact-f32 launches
    assert [o.k for o in base._ops[:3]] == [7, 3, 3]
    assert all(base._op_dtype(o) == L.PPN_F32 for o in base._ops[:3])
    assert (stem.out_raw, stem.out_act, stem.bn2) == (base._ops[2].out_raw, base._ops[2].out_act, base._ops[2].bn2)
    # one stem launch instead of three; everything behind it unchanged
    assert len(fused._ops) == len(base._ops) - 2
    assert [_sig(fused, o) for o in fused._ops[1:]] == [_sig(base, o) for o in base._ops[3:]]
    assert sum(1 for o in fused._ops if o.k == 7) == 1


def test_fused_x3_stem_defaults_unchanged():
    for kw in (dict(compute_dtype="float16x3"), dict(compute_dtype="float16", exact_prefix=3)):
        for fs in (None, False):
            net = model.PoseProposalNet("drn_d_22", fuse_stem=fs, **kw)
            assert net._ops[0].next3x3 is None and net._ops[0].next_s2 is None
    net = model.PoseProposalNet("drn_d_22", compute_dtype="float16", exact_prefix=3, fuse_stem=True)
    assert net._ops[0].next3x3 is not None and net._ops[0].next_s2 is None
    assert net._op_dtype(net._ops[0]) == L.PPN_F32


def test_fused_stem_still_rejected_where_it_was():
    with pytest.raises(ValueError):
        model.PoseProposalNet("drn_d_22", compute_dtype="float32", fuse_stem="all")
    with pytest.raises(ValueError):
        model.PoseProposalNet("drn_d_22", compute_dtype="float16x3", fuse_stem=True)
    with pytest.raises(ValueError):
        model.PoseProposalNet("drn_d_22", compute_dtype="float16x3", fuse_stem="all", fuse_shortcut=True)


def test_stem_io_dtype_value():
    assert L.PPN_STEM_X3_F32 == L.PPN_STEM_IO(L.PPN_F16X3, L.PPN_F32) == 0x103
