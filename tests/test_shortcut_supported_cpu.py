"""Host logic of the shortcut fusion (include/xv2.h "shortcut fusion") without a GPU: the shape rule of
xv2_bn_act_shortcut_supported, the workspace size and the argument checks of the two entry points."""
import pytest

F32, BF16 = 0, 1


def _rule(npix, C, dtype):
    """the documented rule: the vector path of the column sums - 4 channels per lane, a block row covers all C channels (C / 4
    lanes divide the 256 threads) or 256-channel groups (C a multiple of 256)"""
    if npix <= 0 or C <= 0 or dtype not in (F32, BF16) or C % 4:
        return 0
    return 1 if (C % 256 == 0 or (C // 4 <= 256 and 256 % (C // 4) == 0)) else 0


def test_supported_follows_the_shape_rule():
    from xview2_amd._capi import query
    seen = set()
    for C in list(range(-4, 300)) + [320, 384, 512, 640, 768, 1000, 1024, 1280, 2048, 2052, 4096]:
        for npix in (0, 1, 32, 1517, 2 * 1024 * 1024):
            for dtype in (F32, BF16, 2):
                got = query("xv2_bn_act_shortcut_supported", npix, C, dtype)
                assert got == _rule(npix, C, dtype), (npix, C, dtype, got)
                seen.add(got)
    assert seen == {0, 1}
    # the encoders' projection shortcuts (resnet50 / ResNeSt: 256 .. 2048 channels) have the fused form; C = 96 has none
    assert all(query("xv2_bn_act_shortcut_supported", 2048, C, F32) == 1 for C in (64, 256, 512, 1024, 2048))
    assert query("xv2_bn_act_shortcut_supported", 2048, 96, F32) == 0


def _chunks(npix, C):
    """chunk_geom's rule (csrc/norm_act.hip) for the vector path"""
    groups = C // 256 if (C > 256 and C % 256 == 0) else 1
    rpp = 256 // ((C // groups) // 4)
    rpb = -(-npix * groups // 2048)
    rpb = max(-(-rpb // rpp) * rpp, rpp * 8)
    return -(-npix // rpb)


@pytest.mark.parametrize("npix,C", [(32, 64), (1517, 256), (8192, 512), (34816, 256), (2 * 256 * 256, 256)])
def test_workspace_holds_partials_and_scratch_rows_of_both_layers(npix, C):
    from xview2_amd._capi import query
    need = _chunks(npix, C) * 2 * C * 2 * 8 + 64 * 2 * C * 2 * 8      # [chunks][2C][2] doubles + XV2_BN_SCRATCH_ROWS rows of 2C
    got = query("xv2_bn_act_shortcut_backward_workspace", npix, C)
    assert need <= got <= need + 16, (got, need)
    assert query("xv2_bn_act_shortcut_backward_workspace", 0, C) == 0


def test_entry_points_reject_bad_arguments_before_any_launch():
    from xview2_amd import _capi, _lib
    fwd = _capi._func("xv2_bn_act_shortcut_forward")
    bwd = _capi._func("xv2_bn_act_shortcut_backward")
    err = _lib.lib().xv2_last_error
    p = 4096          # (never dereferenced: every case below fails its argument check)
    assert fwd(None, p, p, p, p, p, 1, p, p, 32, 64, F32, None) == 1 and b"null argument" in err()
    assert fwd(p, p, p, p, p, p, 3, p, p, 32, 64, F32, None) == 1 and b"ReLU-type" in err()
    assert fwd(p, p, p, p, p, p, 1, p, p, 32, 96, F32, None) == 1 and b"no fused form" in err()
    assert fwd(p, p, p, p, p, p, 1, p, p, 32, 64, 7, None) == 1 and b"dtype" in err()
    assert fwd(p + 4, p, p, p, p, p, 1, p, p, 32, 64, F32, None) == 1 and b"unaligned" in err()
    args = [p, p, p, p, p, p, p, p, p, p, 1, 32.0, p, p, 32, 64, p, p, p, p, p, None, p, F32, None]
    bad = list(args)
    bad[1] = None                                        # the byte mask
    assert bwd(*bad) == 1 and b"null argument" in err()
    bad = list(args)
    bad[10] = 0                                          # no activation
    assert bwd(*bad) == 1 and b"ReLU-type" in err()
    bad = list(args)
    bad[15] = 96
    assert bwd(*bad) == 1 and b"no fused form" in err()
    bad = list(args)
    bad[12] = p + 8                                      # dy3 off a 16-byte boundary
    assert bwd(*bad) == 1 and b"unaligned" in err()
