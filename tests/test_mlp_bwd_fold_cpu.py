"""Host-side argument checks of the entry points behind the folded shared-MLP backward (mgar_bn_act_maxpool_bwd_reduce,
mgar_pointwise_conv_fwd_maxgrad, mgar_pointwise_conv_dw_maxgrad).  They run before any HIP call, so no GPU is needed: bad
arguments come back as codes (-1 MGAR_EINVAL, -3 MGAR_EUNSUPPORTED), never as a launch."""
import ctypes

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
P1 = 0x1000   # a non-null pointer that must never be dereferenced by a check


def _fn(name):
    from multimodal_gar_amd import _lib
    return _lib._fns[name], _lib._cdll.mgar_last_error


def test_signatures_follow_the_header():
    from multimodal_gar_amd import _lib
    I, LL, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    expect = {
        "mgar_bn_act_maxpool_bwd_reduce": [P, LL, LL, LL, P, P, P, P, I, I, I, I, P, P, I, P, P, P, P, P, P],
        "mgar_pointwise_conv_fwd_maxgrad": [P, I, I, I, I, P, I, I, I, P, P, P, P, P, P, P, P],
        "mgar_pointwise_conv_dw_maxgrad": [P, P, I, I, I, I, I, P, P, P, P, I, P, P, P, P, P, P, P, P, P],
    }
    for name, argtypes in expect.items():
        fn = _lib._fns[name]
        assert fn.restype is I and list(fn.argtypes) == argtypes, name
    assert _lib.ABI_VERSION >= 15


def test_maxpool_bwd_reduce_checks_its_arguments():
    fn, err = _fn("mgar_bn_act_maxpool_bwd_reduce")

    def call(dpool=P1, sb=0, sc=-1, sm=1, pooled=P1, arg=P1, x=P1, xarg=None, B=2, C=8, M=16, ns=16, mean=P1, invstd=P1, relu=1,
             ws=P1, dgamma=None, dbeta=None, coef=P1, dmask=P1):
        return fn(dpool, sb, sc, sm, pooled, arg, x, xarg, B, C, M, ns, mean, invstd, relu, ws, dgamma, dbeta, coef, dmask, None)

    assert call(B=-1) == EINVAL and b"bad sizes" in err()
    assert call(ns=0) == EINVAL and call(ns=256) == EINVAL
    assert call(sc=3, sm=0) == EINVAL and b"strides" in err()
    assert call(sb=-1, sc=1, sm=8) == EINVAL
    assert call(B=0) == OK and call(M=0) == OK                    # empty is a no-op, whatever the pointers
    for missing in ("dpool", "pooled", "arg", "mean", "invstd", "ws", "coef", "dmask"):
        assert call(**{missing: None}) == EINVAL and b"null pointer" in err(), missing
    assert call(x=None, xarg=None) == EINVAL                      # the arg-max value comes from one of the two
    assert call(C=70000) == EINVAL


def test_pointwise_conv_fwd_maxgrad_checks_its_arguments():
    fn, err = _fn("mgar_pointwise_conv_fwd_maxgrad")

    def call(x4=P1, B=2, Cin=32, M=64, ns=16, w=P1, rs=1, cs=16, Cout=16, mean=P1, invstd=P1, gamma=None, coef=P1, arg=P1,
             dmask=P1, y=P1):
        return fn(x4, B, Cin, M, ns, w, rs, cs, Cout, mean, invstd, gamma, coef, arg, dmask, y, None)

    assert call(B=-1) == EINVAL and call(M=-1) == EINVAL and call(ns=0) == EINVAL and call(ns=256) == EINVAL
    assert call(M=1 << 27, ns=16) == EINVAL and b"too large" in err()      # M * ns must stay a 32-bit column index
    assert call(B=0) == OK and call(M=0) == OK and call(Cout=0) == OK
    for missing in ("x4", "w", "y", "mean", "invstd", "coef", "arg", "dmask"):
        assert call(**{missing: None}) == EINVAL and b"null pointer" in err(), missing
    assert call(ns=6) == EUNSUPPORTED and b"nsample % 4" in err()
    assert call(ns=18) == EUNSUPPORTED
    assert call(Cin=65) == EUNSUPPORTED and call(Cout=65) == EUNSUPPORTED and call(Cin=0) == EUNSUPPORTED


def test_pointwise_conv_dw_maxgrad_checks_its_arguments():
    fn, err = _fn("mgar_pointwise_conv_dw_maxgrad")

    def call(x=P1, x4=P1, B=2, Cin=16, Cout=32, M=64, ns=16, in_mean=P1, in_invstd=P1, in_gamma=None, in_beta=None, in_relu=1,
             mean=P1, invstd=P1, gamma=None, coef=P1, arg=P1, dmask=P1, ws=P1, dw=P1):
        return fn(x, x4, B, Cin, Cout, M, ns, in_mean, in_invstd, in_gamma, in_beta, in_relu, mean, invstd, gamma, coef, arg, dmask,
                  ws, dw, None)

    assert call(B=-1) == EINVAL and call(Cin=-1) == EINVAL and call(ns=0) == EINVAL and call(ns=256) == EINVAL
    assert call(M=1 << 27, ns=16) == EINVAL and b"too large" in err()
    assert call(Cin=0) == OK and call(Cout=0) == OK
    assert call(dw=None) == EINVAL and b"null pointer" in err()
    assert call(in_invstd=None) == EINVAL and b"in_mean without in_invstd" in err()
    assert call(ns=6) == EUNSUPPORTED and b"nsample % 4" in err()
    assert call(Cin=65) == EUNSUPPORTED and call(Cout=65) == EUNSUPPORTED
    for missing in ("x", "x4", "ws", "mean", "invstd", "coef", "arg", "dmask"):
        assert call(**{missing: None}) == EINVAL and b"null pointer" in err(), missing
