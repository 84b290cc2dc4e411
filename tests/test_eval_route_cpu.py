"""multimodal_gar_amd/eval_route.py on its own: the version-keyed cache every eval-mode route keeps its derived tensors in, and
the three atoms of the plan predicates.  Host only."""
import copy
import gc
import types
import weakref

import torch
import torch.nn as nn

from multimodal_gar_amd import eval_route as R

SLOT = "_mgar_test_slot"


class _Counted:
    """a build function that doubles the module's weight and counts its calls"""

    def __init__(self, lin):
        self.lin, self.calls = lin, 0

    def __call__(self):
        self.calls += 1
        return self.lin.weight.detach() * 2.0


def _get(lin, build, **kw):
    return R.cached(lin, SLOT, (lin.weight,), build, **kw)


def test_second_call_returns_the_identical_object_and_the_slot_layout():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    a = _get(lin, build)
    assert _get(lin, build) is a and build.calls == 1
    assert torch.equal(a, lin.weight.detach() * 2.0)
    entry = lin.__dict__[SLOT]
    assert isinstance(entry, tuple) and entry[1] is a and hash(entry[0]) is not None
    assert SLOT not in lin.state_dict() and set(lin.state_dict()) == {"weight", "bias"}


def test_every_change_of_a_read_tensor_rebuilds():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    last = _get(lin, build)

    def rebuilt(n):
        nonlocal last
        new = _get(lin, build)
        assert new is not last and build.calls == n and torch.equal(new, lin.weight.detach() * 2.0)
        assert _get(lin, build) is new and build.calls == n
        last = new

    with torch.no_grad():
        lin.weight.mul_(3.0)                                    # an in-place update
    rebuilt(2)
    lin.weight.data = torch.ones(4, 3)                          # a replaced .data
    rebuilt(3)
    lin.weight = nn.Parameter(torch.full((4, 3), 5.0))          # a replaced parameter object
    rebuilt(4)
    lin.double()                                                # dtype (Module._apply swaps .data)
    rebuilt(5)
    assert last.dtype == torch.float64


def test_device_and_dtype_are_in_the_key_on_their_own():
    """Two tensors that agree in _version and data_ptr() and differ in dtype only -- a view of the same storage -- do not match."""
    owner = types.SimpleNamespace()
    t = torch.zeros(4, dtype=torch.float32)
    v = t.view(torch.int32)
    assert (t._version, t.data_ptr(), t.device) == (v._version, v.data_ptr(), v.device)
    a = R.cached(owner, SLOT, (t,), lambda: object())
    assert R.cached(owner, SLOT, (t,), lambda: object()) is a
    b = R.cached(owner, SLOT, (v,), lambda: object())
    assert b is not a
    assert owner.__dict__[SLOT][0][1] == ((v._version, v.data_ptr(), v.device, torch.int32),)


def test_extra_key_parts():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    a = _get(lin, build, extra=(1e-3,))
    assert _get(lin, build, extra=(1e-3,)) is a
    b = _get(lin, build, extra=(1e-5,))
    assert b is not a and build.calls == 2
    assert _get(lin, build) is not b and build.calls == 3      # no extra part is another key too


def test_a_dict_as_owner_is_a_per_prefix_store():
    lin = nn.Linear(3, 4)
    store = {}
    a = R.cached(store, "", (lin.weight,), lambda: object())
    b = R.cached(store, "SG_", (lin.weight,), lambda: object())
    assert a is not b and store[""][1] is a and store["SG_"][1] is b
    assert R.cached(store, "", (lin.weight,), lambda: object()) is a


class _Obj:
    pass


def test_derived_from_identity_rebuilds_and_the_slot_keeps_the_originals_alive():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    first, second = _Obj(), _Obj()
    refs = [weakref.ref(first), weakref.ref(second)]
    a = _get(lin, build, derived_from=(first, second))
    assert _get(lin, build, derived_from=(first, second)) is a and build.calls == 1
    third = _Obj()
    b = _get(lin, build, derived_from=(first, third))            # one identity changed
    assert b is not a and build.calls == 2
    del second
    gc.collect()
    assert refs[1]() is None                                     # the replaced entry let go of what only it held
    ref_third = weakref.ref(third)
    del first, third
    gc.collect()
    assert refs[0]() is not None and ref_third() is not None     # held by the slot: their ids cannot be reused while the key has them
    assert _get(lin, build, derived_from=(refs[0](), ref_third())) is b and build.calls == 2
    del lin.__dict__[SLOT]
    gc.collect()
    assert refs[0]() is None and ref_third() is None


def test_build_runs_without_grad_and_without_autocast():
    lin = nn.Linear(3, 4)
    seen = {}

    def build():
        seen["grad"] = torch.is_grad_enabled()
        seen["autocast"] = torch.is_autocast_enabled("cpu")
        return lin.weight @ lin.weight.t()                       # a matmul: bf16 under CPU autocast, with a grad_fn in grad mode

    with torch.enable_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        assert torch.is_grad_enabled() and torch.is_autocast_enabled("cpu")
        y = _get(lin, build)
        assert torch.is_grad_enabled() and torch.is_autocast_enabled("cpu")      # the caller's modes are back
    assert seen == {"grad": False, "autocast": False}
    assert y.dtype == torch.float32 and not y.requires_grad and y.grad_fn is None


def test_deepcopy_rebuilds_once_and_agrees():
    lin = nn.Linear(3, 4)
    a = _get(lin, _Counted(lin))
    twin = copy.deepcopy(lin)
    build = _Counted(twin)
    b = _get(twin, build)
    assert build.calls == 1 and b is not a and torch.equal(a, b)
    assert _get(twin, build) is b and build.calls == 1
    assert _get(lin, _Counted(lin)) is a                         # the original's entry is untouched
    assert SLOT not in twin.state_dict()


# ---- the atoms ------------------------------------------------------------------------------------------------------------------
def test_hooked_truth_table():
    a, b = nn.ReLU(), nn.Linear(2, 2)
    assert R.hooked() is False and R.hooked(a) is False and R.hooked(a, b) is False
    for register in ("register_forward_hook", "register_forward_pre_hook"):
        handle = getattr(b, register)(lambda *args: None)
        assert R.hooked(b) is True and R.hooked(a, b) is True and R.hooked(b, a) is True and R.hooked(a) is False
        handle.remove()
        assert R.hooked(a, b) is False
    handle = b.register_full_backward_hook(lambda *args: None)   # not a forward hook: it never sees a forward, fused or not
    assert R.hooked(b) is False
    handle.remove()


def test_bn_frozen_truth_table():
    for bn in (nn.BatchNorm1d(4), nn.BatchNorm3d(4, affine=False)):
        assert R.bn_frozen(bn) is False                          # training
        bn.eval()
        assert R.bn_frozen(bn) is True
        mean, var = bn.running_mean, bn.running_var
        bn.running_mean = None
        assert R.bn_frozen(bn) is False
        bn.running_mean, bn.running_var = mean, None
        assert R.bn_frozen(bn) is False
        bn.running_var = var
        assert R.bn_frozen(bn) is True
        bn.train()
        assert R.bn_frozen(bn) is False
    nostat = nn.BatchNorm1d(4, track_running_stats=False).eval()
    assert R.bn_frozen(nostat) is False                          # no running statistics at all
    nostat.running_mean, nostat.running_var = torch.zeros(4), torch.ones(4)
    assert R.bn_frozen(nostat) is True                           # track_running_stats itself is the call site's condition


def test_needs_grad_truth_table():
    def x(rg):
        return types.SimpleNamespace(requires_grad=rg)           # nothing but the attribute is read

    on, off = nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(2), requires_grad=False)
    for grad_mode in (True, False):
        with torch.set_grad_enabled(grad_mode):
            for x_rg in (True, False):
                for params, any_rg in (((), False), ((off,), False), ((on,), True), ((off, on), True), ((None, off), False),
                                       ((None, on), True)):
                    assert R.needs_grad(x(x_rg), params) is (grad_mode and (x_rg or any_rg)), (grad_mode, x_rg, params)
                assert R.needs_grad(x(x_rg)) is (grad_mode and x_rg)
                assert R.needs_grad(x(x_rg), (p for p in (off, on))) is grad_mode      # a generator is an iterable like another
    assert R.needs_grad(torch.zeros(2, requires_grad=True), [off]) is True


def test_needs_grad_leaves_the_iterable_alone_when_grad_mode_is_off():
    def params():
        raise AssertionError("consumed")
        yield

    with torch.no_grad():
        assert R.needs_grad(types.SimpleNamespace(requires_grad=True), params()) is False
