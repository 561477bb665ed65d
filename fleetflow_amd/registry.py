"""Control-plane server registry -> planner node table.

fleetflowd lists a tenant's servers with
``SELECT * FROM server WHERE tenant.slug = $t AND deleted_at IS NONE ORDER BY slug``
(crates/fleetflow-controlplane/src/db.rs:741-750). Each row carries optional
``capacity``/``allocated`` (model.rs:414-427), ``labels`` (model.rs:399-411) and
``scheduling`` (model.rs:435-442). The planner's node index is the position in
that slug order. The conversion is SPEC.md 4:

* ``cpu_free = (capacity.cpu_cores - allocated.cpu_cores) * 1000`` millicores;
* ``mem_free = (capacity.memory_gb - allocated.memory_gb) * 1024`` MiB;
* a missing capacity falls back to the plan string (``parse_plan``,
  crates/fleetflow-cloud-sakura/src/provider.rs:15-30), and a row with neither is
  unconstrained;
* ``scheduling`` other than "schedulable" (cordon, drain) makes the node
  unschedulable; None means schedulable (model.rs:516-518); "drain" also sets
  ``Server.draining``, which ``flow.drain_stage`` reads (SPEC.md 2.11);
* labels become ``key=value`` strings (tier, region, class, arch, then the
  ``extras`` object), mapped to bits by ``flow.LabelDict``.
"""
from __future__ import annotations

from .flow import POLICY_STRATEGIES, U32_MAX, PlacementPolicy, Server

SCHEDULABLE, CORDON, DRAIN = "schedulable", "cordon", "drain"


def _rust_i32(s: str):
    """``str::parse::<i32>()``: optional sign, ASCII digits only, in range."""
    if not s:
        return None
    body = s[1:] if s[0] in "+-" else s
    if not body or not all("0" <= ch <= "9" for ch in body):
        return None
    v = int(s)
    return v if -(2 ** 31) <= v < 2 ** 31 else None


def _trim_end_matches(s: str, suffix: str) -> str:
    while suffix and s.endswith(suffix):
        s = s[:-len(suffix)]
    return s


def parse_plan(plan: str | None) -> tuple[int, int]:
    """provider.rs:15-30: ``"Ncore-Mgb"`` -> (N, M); any part that does not parse
    is 1, and anything but exactly two ``-`` parts is (1, 1)."""
    if plan is not None:
        parts = plan.split("-")
        if len(parts) == 2:
            core = _rust_i32(_trim_end_matches(parts[0], "core"))
            mem = _rust_i32(_trim_end_matches(parts[1], "gb"))
            return (1 if core is None else core, 1 if mem is None else mem)
    return (1, 1)


def _clamp_u32(v: int) -> int:
    return 0 if v < 0 else min(v, U32_MAX)


def server_labels(labels: dict | None) -> list[str]:
    if not labels:
        return []
    out = [f"{k}={labels[k]}" for k in ("tier", "region", "class", "arch") if labels.get(k) is not None]
    extras = labels.get("extras")
    if isinstance(extras, dict):
        out += [f"{k}={v}" for k, v in sorted(extras.items()) if isinstance(v, (str, int, float, bool))]
    return out


def server_from_row(row: dict) -> Server:
    """One registry ``server`` row (as JSON) -> planner node."""
    cap = row.get("capacity") or {}
    alloc = row.get("allocated") or {}
    cc, cm = cap.get("cpu_cores"), cap.get("memory_gb")
    if cc is None or cm is None:
        if row.get("plan") is not None:
            pc, pm = parse_plan(row["plan"])
            cc = pc if cc is None else cc
            cm = pm if cm is None else cm
    cpu = U32_MAX if cc is None else _clamp_u32((cc - (alloc.get("cpu_cores") or 0)) * 1000)
    mem = U32_MAX if cm is None else _clamp_u32((cm - (alloc.get("memory_gb") or 0)) * 1024)
    sched = row.get("scheduling")
    return Server(slug=row["slug"], cpu_m=cpu, mem_mib=mem, labels=server_labels(row.get("labels")),
                  schedulable=sched is None or sched == SCHEDULABLE, provider=row.get("provider", ""),
                  plan=row.get("plan"), draining=sched == DRAIN)


def plan_template(plan: str | None, labels: dict | None = None, name: str | None = None) -> Server:
    """A server template for ``flow.grow_stage`` (SPEC.md 2.12) from a provider plan string: ``parse_plan``'s
    cores * 1000 millicores and GB * 1024 MiB (provider.rs:15-30), and the ServerLabels a new server of the
    plan would carry (model.rs:399-411) as ``server_labels`` renders them.  ``name`` defaults to the plan
    string."""
    cores, gb = parse_plan(plan)
    return Server(slug=name if name is not None else str(plan), cpu_m=_clamp_u32(cores * 1000),
                  mem_mib=_clamp_u32(gb * 1024), labels=server_labels(labels), plan=plan)


def node_table(rows: list[dict]) -> list[Server]:
    """db.rs:741-750: live rows (``deleted_at`` None) in slug order."""
    live = [r for r in rows if r.get("deleted_at") is None]
    return [server_from_row(r) for r in sorted(live, key=lambda r: r["slug"])]


def placement_policy(tenant_row: dict | None) -> PlacementPolicy | None:
    """A tenant row's ``placement_policy`` (as JSON; model.rs:82-95) -> the planner's policy: its
    ``strategy`` constant, soft ``preferred_labels`` map, hard ``spread_constraint``
    (``topology_key``, ``max_skew``; SPEC.md 2.7) and ``fallback_policy`` (``relax_order``, ``max_hops``;
    SPEC.md 2.8) and ``resource_quota`` (SPEC.md 2.10): ``cpu_cores`` * 1000 millicores, ``memory_gb`` * 1024
    MiB and ``max_services_per_stage`` as it is; a missing or null field is no cap, and a value past what a
    u32 cap can say (0xFFFFFFFE) is no cap either.  The quota's ``max_stages`` is not read: it caps the
    tenant's stage records, not a stage's placement.  None when the row has no policy; a strategy that is
    none of the three constants, a constraint with a key and a ``max_skew`` below 1, a ``relax_order`` that
    is no list of label keys, a ``max_hops`` that is no integer >= 0, a chain of more than four effective
    hops, or a quota field that is negative or no integer is a ValueError."""
    pol = (tenant_row or {}).get("placement_policy")
    if pol is None:
        return None
    strategy = pol.get("strategy")
    if strategy is not None and strategy not in POLICY_STRATEGIES:
        raise ValueError(f"unknown placement strategy {strategy!r} (expected {'|'.join(POLICY_STRATEGIES)})")
    pref = pol.get("preferred_labels") or {}
    spread = pol.get("spread_constraint") or {}
    key, skew = spread.get("topology_key"), spread.get("max_skew")
    if key is not None:
        if isinstance(skew, bool) or not isinstance(skew, int) or not 1 <= skew <= U32_MAX:
            raise ValueError(f"spread_constraint on '{key}': max_skew must be an integer in 1..{U32_MAX}, got {skew!r}")
        key = str(key)
    else:
        skew = None
    fb = pol.get("fallback_policy") or {}
    if not isinstance(fb, dict):
        raise ValueError(f"fallback_policy must be an object with relax_order and max_hops, got {fb!r}")
    order, hops = fb.get("relax_order") or (), fb.get("max_hops")
    if isinstance(order, str) or not all(isinstance(k, str) for k in order):
        raise ValueError(f"fallback_policy: relax_order must be a list of label keys, got {order!r}")
    rq = pol.get("resource_quota") or {}
    if not isinstance(rq, dict):
        raise ValueError(f"resource_quota must be an object, got {rq!r}")
    caps = []
    for name, scale in (("cpu_cores", 1000), ("memory_gb", 1024), ("max_services_per_stage", 1)):
        v = rq.get(name)
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
            raise ValueError(f"resource_quota: {name} must be an integer >= 0 or null, got {v!r}")
        # a cap too large for the u32 of the ABI cannot bind before the usage wraps: no cap
        caps.append(None if v is None or v * scale >= U32_MAX else v * scale)
    return PlacementPolicy(strategy, {str(k): str(v) for k, v in pref.items()}, key, skew, tuple(order), hops, *caps)


def pool_required_labels(pool: dict | None) -> list[str]:
    """WorkerPool.required_labels (model.rs:557-558) -> required ``key=value`` labels."""
    req = (pool or {}).get("required_labels") or {}
    return [f"{k}={v}" for k, v in sorted(req.items())]
