"""What every eval-mode route shares on the host: the cache of tensors derived from a module's
parameters, and the atoms of the plan predicates.  No kernel calls; imports nothing but torch."""
import torch


def cached(owner, slot, read, build, extra=(), derived_from=()):
    """build() once per state of what it reads, kept in owner.__dict__[slot] (``owner``: an nn.Module, or a plain dict for a
    per-prefix store) as (key, value, derived_from); tests and callers may look at [0] and [1].  Never in state_dict().

    The key covers (_version, data_ptr(), device, dtype) of every tensor in ``read`` -- an in-place update, a replaced .data or
    parameter, .to() / .double() all rebuild --, the hashable ``extra`` parts (eps, ...) and the IDENTITIES of the
    ``derived_from`` objects: results of another cached() call that build() reads instead of the tensors behind them.  An id
    means something only while its object lives, so the entry holds derived_from for as long as it holds the key: a collected
    object's id can then never be taken by a new one and match a stale entry.  This is the one place that rule lives.

    build() runs under no_grad with autocast off for the device type of read[0] -- ``read`` holds at least one tensor --: the
    value never depends on the caller's mode."""
    store = owner if type(owner) is dict else owner.__dict__
    key = (tuple(extra), tuple([(t._version, t.data_ptr(), t.device, t.dtype) for t in read]), tuple(map(id, derived_from)))
    entry = store.get(slot)
    if entry is not None and entry[0] == key:
        return entry[1]
    with torch.no_grad(), torch.autocast(device_type=read[0].device.type, enabled=False):
        value = build()
    store[slot] = (key, value, tuple(derived_from))
    return value


def hooked(*modules):
    """a forward (pre-)hook sits on one of the modules: a fused route would not run the module the hook wants to see"""
    return any(bool(m._forward_hooks or m._forward_pre_hooks) for m in modules)


def bn_frozen(bn):
    """the BatchNorm is the per-channel affine map of its running statistics: not training, both statistics present"""
    return not bn.training and bn.running_mean is not None and bn.running_var is not None


def needs_grad(x, params=()):
    """autograd would record this call: grad mode is on and x, or a tensor of ``params`` (None entries skipped), requires a
    gradient.  Which parameters count is the caller's choice; a generator is consumed only when grad mode is on."""
    return torch.is_grad_enabled() and bool(x.requires_grad or any(p is not None and p.requires_grad for p in params))
