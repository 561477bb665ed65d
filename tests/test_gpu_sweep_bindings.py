"""GPU tests of the sweep exports' argument handling (fleetflow_amd/csrc/fp_ctx.hip; SPEC.md 2.11, 2.12 and 2.15 to
2.18): the six host-pointer exports and the six fp_dev_* ones, called raw on C = 3, N = 2 and two candidates,
variants or templates.  Each required pointer null in turn is FP_EINVAL; two mistakes in one call return the code
of the check that stands first in the source; every output keeps its sentinel; and after every refused call the
same context takes a valid call.  What the sweeps compute is tested in test_gpu_drain*.py, test_gpu_shrink*.py and
test_gpu_grow*.py."""
import ctypes as ct

import numpy as np
import pytest

from fleetflow_amd import _lib

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NOFIT = 1 << _lib.REASON_NOFIT
OK, EINVAL, EOVERFLOW = _lib.FP_OK, _lib.FP_EINVAL, _lib.FP_EOVERFLOW
C, N, K = 3, 2, 2
CONT = ("cpu_m", "mem_mib", "req_labels", "conflict")
NODE = ("cpu_free", "mem_free", "labels", "conflict_used", "schedulable")
HOST_ONLY = ("relax_mask", "quota", "quota_used")  # host arrays in the fp_dev_* exports too

_DRAIN = ("cs", "ns", "assign", "group", "n_cand", "strategy", "preferred", "node_count")
_SHRINK = ("cs", "ns", "assign", "try_order", "n_var", "n_try", "strategy", "preferred", "node_count")
_CHAIN = ("domain", "max_skew", "relax_mask", "n_hops")
ARGS = {
    "drain_sweep": _DRAIN + ("assign_out", "reason_out", "summary_out"),
    "drain_sweep_policy": _DRAIN + _CHAIN + ("assign_out", "reason_out", "hops_out", "summary_out", "policy_out"),
    "shrink_sweep": _SHRINK + ("assign_out", "state_out", "blocker_out", "summary_out"),
    "shrink_sweep_policy": _SHRINK + _CHAIN + ("assign_out", "state_out", "blocker_out", "summary_out", "hops_out",
                                               "blocker_reason_out", "policy_out"),
    "grow_sweep": ("cs", "reason", "reason_mask", "n_cand", "t_cpu", "t_mem", "t_labels", "t_max", "max_new",
                   "summary_out", "assign_out"),
    "grow_sweep_policy": ("cs", "reason", "reason_mask", "ns", "node_count", "n_cand", "t_cpu", "t_mem", "t_labels",
                          "t_max", "max_new", "strategy", "preferred", "domain", "t_domain", "max_skew", "relax_mask",
                          "n_hops", "quota", "quota_used", "summary_out", "policy_out", "assign_out", "hops_out",
                          "reason_out"),
}
# the outputs of each family: name -> (dtype, entries)
OUTS = {
    "drain": dict(assign_out=(np.uint32, C), reason_out=(np.uint8, C), summary_out=(np.uint32, K * 8),
                  hops_out=(np.uint8, C), policy_out=(np.uint32, K * 4)),
    "shrink": dict(assign_out=(np.uint32, K * C), state_out=(np.uint8, K * N), blocker_out=(np.uint32, K * N),
                   summary_out=(np.uint32, K * 8), hops_out=(np.uint8, K * C), blocker_reason_out=(np.uint8, K * N),
                   policy_out=(np.uint32, K * 4)),
    "grow": dict(summary_out=(np.uint32, K * 8), policy_out=(np.uint32, K * 8), assign_out=(np.uint32, K * C),
                 hops_out=(np.uint8, K * C), reason_out=(np.uint8, K * C)),
}
# the pointers each export refuses when null (everything else is optional)
REQUIRED = {
    "drain": CONT + NODE + ("assign", "group", "assign_out", "reason_out", "summary_out"),
    "shrink": CONT + NODE + ("assign", "try_order", "assign_out", "state_out", "summary_out"),
    "grow_sweep": CONT + ("reason", "t_cpu", "t_mem", "t_labels", "summary_out"),
    "grow_sweep_policy": CONT + NODE + ("reason", "t_cpu", "t_mem", "t_labels", "summary_out", "domain"),
}
EXPORTS = [(name, dev) for name in ARGS for dev in (False, True)]


def _u32(*x):
    return np.array(x, np.uint32)


def _values(n_nodes=N):
    """A valid call's arguments by name (numpy arrays and ints)."""
    v = dict(cpu_m=_u32(1, 1, 1), mem_mib=_u32(1, 1, 1), req_labels=_u32(0, 0, 0), conflict=_u32(0, 0, 0),
             cpu_free=np.full(n_nodes, 9, np.uint32), mem_free=np.full(n_nodes, 9, np.uint32),
             labels=np.zeros(n_nodes, np.uint32), conflict_used=np.zeros(n_nodes, np.uint32),
             schedulable=np.ones(n_nodes, np.uint8), n_containers=C, n_nodes=n_nodes,
             assign=_u32(0, 1, NONE), group=np.arange(n_nodes, dtype=np.uint32) % K, try_order=_u32(0, 1, 1, NONE),
             n_cand=K, n_var=K, n_try=2, strategy=0, preferred=0, node_count=np.zeros(n_nodes, np.uint32),
             domain=np.arange(n_nodes, dtype=np.uint32) % 2, max_skew=1, relax_mask=_u32(1, 0, 0, 0), n_hops=1,
             reason=np.full(C, _lib.REASON_NOFIT, np.uint8), reason_mask=NOFIT, t_cpu=_u32(4, 8), t_mem=_u32(4, 8),
             t_labels=_u32(0, 0), t_max=_u32(1, 1), max_new=2, t_domain=_u32(0, 1), quota=_u32(100, 100, 100),
             quota_used=_u32(0, 0, 0))
    return v


class _Call:
    """One raw call of an export: the arguments of ``_values`` with ``over`` on top (None = a null pointer), every
    output prefilled with 0xA5.  ``rc`` is the export's return value."""

    def __init__(self, planner, name, dev, n_nodes=N, **over):
        import torch
        family = name.split("_")[0]
        self.planner, self.dev = planner, dev
        export = ("fp_dev_" if dev else "fp_") + name
        v = _values(n_nodes)
        for k, (dtype, n) in OUTS[family].items():
            v[k] = np.full(n * np.dtype(dtype).itemsize, 0xA5, np.uint8).view(dtype)
        v.update(over)
        self.outs = {k: v[k] for k in OUTS[family] if k in ARGS[name] and v[k] is not None}
        self.keep = []  # whatever the addresses sent point into

        def address(key):
            a = v[key]
            if a is None:
                return None
            if dev and key not in HOST_ONLY:
                t = torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8).copy()).to("cuda:0")
                if key in self.outs:
                    self.outs[key] = t
                a = t
            self.keep.append(a)
            return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data

        cs = _lib.FpContainers(v["n_containers"], *(address(k) for k in CONT))
        ns = _lib.FpNodes(v["n_nodes"], *(address(k) for k in NODE))
        args = [planner._ctx]
        for key, ctype in zip(ARGS[name], _lib.SIGNATURES[export][1][1:]):
            if key in ("cs", "ns"):
                args.append(ct.byref(cs if key == "cs" else ns))
            elif ctype is ct.c_uint32:
                args.append(v[key])
            else:
                a = address(key)
                args.append(None if a is None else ct.cast(ct.c_void_p(a), ctype))
        assert len(args) == len(_lib.SIGNATURES[export][1])
        if dev:
            torch.cuda.synchronize()  # the copies to the device are done before the context's stream reads them
        self.rc = getattr(planner._L, export)(*args)

    def untouched(self):
        if self.dev:
            self.planner.sync()
        return all(bool((np.asarray(o.cpu() if self.dev else o).view(np.uint8) == 0xA5).all())
                   for o in self.outs.values())


def _refused(planner, name, dev, code, what, **over):
    call = _Call(planner, name, dev, **over)
    assert call.rc == code, (name, dev, what, call.rc)
    assert call.untouched(), (name, dev, what)
    good = _Call(planner, name, dev)  # the context goes on
    assert good.rc == OK, (name, dev, what, "the valid call after it")
    if dev:
        planner.sync()
    assert not good.untouched(), (name, dev, what)


@pytest.mark.parametrize("name,dev", EXPORTS)
def test_a_valid_call_writes_every_output(planner, name, dev):
    call = _Call(planner, name, dev)
    assert call.rc == OK
    if dev:
        planner.sync()
    for key, o in call.outs.items():
        assert not (np.asarray(o.cpu() if dev else o).view(np.uint8) == 0xA5).all(), key


@pytest.mark.parametrize("name,dev", EXPORTS)
def test_null_arguments(planner, name, dev):
    family = name.split("_")[0]
    for key in REQUIRED[name if family == "grow" else family]:
        _refused(planner, name, dev, EINVAL, key, **{key: None})


@pytest.mark.parametrize("name,dev", EXPORTS)
def test_precedence_of_two_mistakes(planner, name, dev):
    """The expected codes follow the order of the checks in fp_ctx.hip and in the *_impl functions as they stood
    when every export had its own copy."""
    family, policy = name.split("_")[0], name.endswith("_policy")
    if family in ("drain", "shrink"):
        # the node count is tested before the strategy, and the strategy before the tables
        _refused(planner, name, dev, EOVERFLOW, "N and strategy", n_nodes=8193, strategy=4)
        _refused(planner, name, dev, EINVAL, "strategy and a null table", strategy=4, cpu_free=None)
        _refused(planner, name, dev, EINVAL, "strategy and a null assign", strategy=4, assign=None)
        if policy:
            # the device export tests n_hops itself, before the sweep's own checks; the host export after them
            _refused(planner, name, dev, EINVAL if dev else EOVERFLOW, "N and n_hops", n_nodes=8193, n_hops=5)
            _refused(planner, name, dev, EINVAL, "n_hops and a null table", n_hops=5, conflict=None)
    if family == "drain":
        _refused(planner, name, dev, EOVERFLOW, "n_cand and strategy", n_cand=8193, strategy=4, summary_out=None)
        # nothing to do is found last: C == 0 and n_cand == 0 with a bad strategy is still refused
        empty = dict(n_containers=0, n_cand=0, group=_u32(NONE, NONE))
        _refused(planner, name, dev, EINVAL, "nothing to do and strategy", strategy=4, **empty)
        call = _Call(planner, name, dev, **empty)
        assert call.rc == OK and call.untouched()
    if family == "shrink":
        # no variant is found after the scalars and before the tables
        nulls = dict(n_var=0, cpu_m=None, schedulable=None, assign=None, summary_out=None)
        call = _Call(planner, name, dev, **nulls)
        assert call.rc == OK and call.untouched()
        _refused(planner, name, dev, EINVAL, "no variant and strategy", strategy=4, **nulls)
        _refused(planner, name, dev, EOVERFLOW, "n_var and strategy", n_var=65536, strategy=4, summary_out=None)
        if policy:
            _refused(planner, name, dev, EINVAL, "no variant and n_hops", n_hops=5, **nulls)
    if family == "grow":
        _refused(planner, name, dev, EOVERFLOW, "max_new and a null reason", max_new=8193, reason=None)
        _refused(planner, name, dev, EOVERFLOW, "n_cand and a null template", n_cand=65536, t_cpu=None, summary_out=None)
        if policy:
            # N + max_new: the device export tests the strategy and n_hops itself, before the sweep's own checks
            _refused(planner, name, dev, EINVAL if dev else EOVERFLOW, "N + max_new and strategy", max_new=8191, strategy=4)
            _refused(planner, name, dev, EINVAL if dev else EOVERFLOW, "N + max_new and n_hops", max_new=8191, n_hops=5)
            _refused(planner, name, dev, EINVAL, "strategy and a null table", strategy=4, labels=None)
