"""Host-side mirror of the reference's plan-path interface.

Names and argument meaning follow the Rust reference so callers (and tests) read
the same:

* ``Service`` / ``Stage`` / ``Flow``: the subset of fleetflow-core's model the
  plan path reads (crates/fleetflow-core/src/model/service.rs:26-70,
  model/stage.rs:48-64, model/flow.rs:15-41), plus the resource-request
  extension of SPEC.md 4 (``cpu_m``/``mem_mib``/labels/ports/anti-affinity).
* ``order_by_dependencies(services, flow)``: engine.rs:64-85, computed by the
  GPU stable partition (fp_legacy_order).
* ``resolve_target_server(flow, stage_name)``: handlers/deploy.rs:390-394,
  computed by GPU FFD placement over the stage's servers with unconstrained
  capacity (every container lands on node 0 == ``servers.first()``).
* ``levelize_stage`` / ``plan_stage``: the new planner outputs (SPEC.md 2).
* ``drain_stage``: which servers, or zones, of a stage that runs as a plan says can be taken out
  (SPEC.md 2.11; the `drain` scheduling state of controlplane model.rs:435-442).
* ``grow_stage``: the new servers of each template of a catalogue that a plan's NOFIT services need
  (SPEC.md 2.12).
* ``replan_stage``: the next plan of a stage that runs as a plan says, every service staying on its server
  while it still fits there (SPEC.md 2.13; `cordon` of model.rs:435-442 "stops new placements, existing
  placements continue").

Strings never cross the C ABI: names are mapped to u32 ids in stage order here.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .planner import NONE, Planner

U32_MAX = 0xFFFFFFFF


@dataclass
class Port:
    """fleetflow_core::Port (model/port.rs); parsed by parser/port.rs."""
    host: int
    container: int
    protocol: str = "tcp"
    host_ip: str | None = None


@dataclass
class Volume:
    """fleetflow_core::Volume (model/volume.rs); parsed by parser/volume.rs."""
    host: str
    container: str
    read_only: bool = False


@dataclass
class Service:
    """fleetflow_core::Service subset (model/service.rs:26-70): the fields the plan
    path and the dry-run presenter read."""
    image: str | None = None
    version: str | None = None
    command: str | None = None
    service_type: str | None = None
    restart: str | None = None
    registry: str | None = None
    ports: list[Port] = field(default_factory=list)
    environment: dict[str, str] = field(default_factory=dict)
    volumes: list[Volume] = field(default_factory=list)
    depends_on: list[str] = field(default_factory=list)
    # SPEC.md 4 resource-request extension (ignored by the reference parser,
    # parser/service.rs:222); absent => unconstrained (0)
    cpu_m: int = 0
    mem_mib: int = 0
    labels: list[str] = field(default_factory=list)      # required "key=value" labels
    anti_affinity: str | None = None

    @property
    def host_ports(self) -> list[int]:
        return [p.host for p in self.ports]

    def merge(self, other: "Service") -> None:
        """model/service.rs:380-428: Options override when set, Vecs when non-empty,
        the environment map is merged with ``other`` winning."""
        for f in ("service_type", "image", "version", "command", "restart", "registry", "anti_affinity"):
            if getattr(other, f) is not None:
                setattr(self, f, getattr(other, f))
        for f in ("ports", "volumes", "depends_on", "labels"):
            if getattr(other, f):
                setattr(self, f, list(getattr(other, f)))
        for f in ("cpu_m", "mem_mib"):
            if getattr(other, f):
                setattr(self, f, getattr(other, f))
        self.environment.update(other.environment)


POLICY_STRATEGIES = ("spread_across_pool", "pack_into_dedicated", "fill_lowest")


@dataclass
class PlacementPolicy:
    """The tenant PlacementPolicy subset the planner reads (controlplane model.rs:56-95): one of the
    three strategy constants (None = first fit), the soft ``preferred_labels`` map and the hard
    ``SpreadConstraint{topology_key, max_skew}`` (model.rs:56-63; SPEC.md 2.7), which constrains when
    both fields are set and ``max_skew`` >= 1, and ``FallbackPolicy{relax_order, max_hops}``
    (model.rs:47-54; SPEC.md 2.8): the label keys a service may give up, in that order, when the pool that
    matches its required labels has no feasible server, and ``ResourceQuota{max_services_per_stage, cpu_cores,
    memory_gb}`` (model.rs:38-45; SPEC.md 2.10) as three optional caps in planner units: ``quota_cpu_m``
    (millicores), ``quota_mem_mib`` (MiB) and ``quota_services`` (services of the stage); None = no cap.
    The quota's max_stages is not read: it caps the tenant's stage records, not a stage's placement
    (DESIGN.md 4.8).  Two policies compare equal on strategy and preferred labels, the fields SPEC.md 2.6
    reads; compare ``spread`` for the constraint, ``fallback`` for the chain and ``quota`` for the caps."""
    strategy: str | None = None
    preferred_labels: dict[str, str] = field(default_factory=dict)
    spread_topology_key: str | None = field(default=None, compare=False)
    spread_max_skew: int | None = field(default=None, compare=False)
    fallback_relax_order: tuple[str, ...] = field(default=(), compare=False)
    fallback_max_hops: int | None = field(default=None, compare=False)
    quota_cpu_m: int | None = field(default=None, compare=False)
    quota_mem_mib: int | None = field(default=None, compare=False)
    quota_services: int | None = field(default=None, compare=False)

    def __post_init__(self):
        if self.strategy is not None and self.strategy not in POLICY_STRATEGIES:
            raise ValueError(f"unknown placement strategy '{self.strategy}' (expected {'|'.join(POLICY_STRATEGIES)})")
        if self.spread_max_skew is not None and not 0 <= self.spread_max_skew <= U32_MAX:
            raise ValueError(f"spread max_skew must be in 0..{U32_MAX}, got {self.spread_max_skew!r}")
        self.fallback_relax_order = tuple(self.fallback_relax_order)
        _ = self.fallback  # validates the chain
        for name in ("quota_cpu_m", "quota_mem_mib", "quota_services"):
            cap = getattr(self, name)
            # U32_MAX itself is the ABI's "no cap" (FP_QUOTA_UNLIMITED): say None for that
            if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or not 0 <= cap < U32_MAX):
                raise ValueError(f"{name} must be an integer in 0..{U32_MAX - 1} or None, got {cap!r}")

    @property
    def quota(self) -> tuple[int | None, int | None, int | None] | None:
        """(cpu millicores, memory MiB, services) when the policy has a cap in some dimension (None in the
        others), else None."""
        caps = (self.quota_cpu_m, self.quota_mem_mib, self.quota_services)
        return caps if any(c is not None for c in caps) else None

    @property
    def fallback(self) -> tuple[str, ...]:
        """The label keys the chain gives up, one per hop: ``relax_order[:max_hops]`` (``max_hops`` None =
        every key).  Empty = no fallback (no keys, or ``max_hops`` 0).  A ``max_hops`` that is no integer
        >= 0, or more than FP_FALLBACK_MAX_HOPS effective hops, is a ValueError."""
        from ._lib import FP_FALLBACK_MAX_HOPS
        hops = self.fallback_max_hops
        if hops is not None and (isinstance(hops, bool) or not isinstance(hops, int) or hops < 0):
            raise ValueError(f"fallback max_hops must be an integer >= 0, got {hops!r}")
        keys = tuple(self.fallback_relax_order)
        if any(not isinstance(k, str) or not k or "=" in k for k in keys):
            raise ValueError(f"fallback relax_order takes label keys (such as \"class\"), got {keys!r}")
        keys = keys if hops is None else keys[:hops]
        if len(keys) > FP_FALLBACK_MAX_HOPS:
            raise ValueError(f"fallback chain of {len(keys)} hops (at most {FP_FALLBACK_MAX_HOPS}): shorten relax_order "
                             "or set max_hops")
        return keys

    @property
    def spread(self) -> tuple[str, int] | None:
        """(topology_key, max_skew) when the policy carries a constraint that constrains, else None."""
        if self.spread_topology_key is None or self.spread_max_skew is None or self.spread_max_skew < 1:
            return None
        return self.spread_topology_key, self.spread_max_skew

    @property
    def preferred(self) -> list[str]:
        """The preferred labels as the ``key=value`` strings of ``LabelDict``."""
        return [f"{k}={v}" for k, v in sorted(self.preferred_labels.items())]

    @property
    def active(self) -> bool:
        return (self.strategy is not None or bool(self.preferred_labels) or self.spread is not None
                or bool(self.fallback) or self.quota is not None)


@dataclass
class Stage:
    """fleetflow_core::Stage (model/stage.rs:48-64), plus the SPEC.md 4 ``placement`` node."""
    services: list[str] = field(default_factory=list)
    servers: list[str] = field(default_factory=list)
    variables: dict[str, str] = field(default_factory=dict)
    registry: str | None = None
    backend: str = "docker"
    placement: PlacementPolicy | None = None


@dataclass
class Server:
    """Node-table entry: KDL ``server`` (parser/cloud.rs:46-140) or a CP registry
    row (controlplane model.rs:399-442 capacity/labels/scheduling)."""
    slug: str
    cpu_m: int = U32_MAX
    mem_mib: int = U32_MAX
    labels: list[str] = field(default_factory=list)
    schedulable: bool = True
    provider: str = ""
    plan: str | None = None
    # scheduling == "drain" (model.rs:435-442): existing placements are to leave as well.  Such a server is
    # unschedulable like a cordoned one; ``drain_stage`` evacuates the servers that carry the flag
    draining: bool = False


@dataclass
class Flow:
    """fleetflow_core::Flow subset (model/flow.rs:15-41)."""
    name: str = ""
    services: dict[str, Service] = field(default_factory=dict)
    stages: dict[str, Stage] = field(default_factory=dict)
    servers: dict[str, Server] = field(default_factory=dict)
    registry: str | None = None
    variables: dict[str, str] = field(default_factory=dict)


_PLANNER: Planner | None = None


def default_planner() -> Planner:
    global _PLANNER
    if _PLANNER is None:
        _PLANNER = Planner(0)
    return _PLANNER


def has_deps_vector(services: list[str], flow: Flow) -> np.ndarray:
    """The engine.rs:71-80 predicate per position: known AND depends_on non-empty."""
    return np.array([1 if (n in flow.services and flow.services[n].depends_on) else 0 for n in services],
                    dtype=np.uint8)


def order_by_dependencies(services: list[str], flow: Flow, planner: Planner | None = None) -> list[str]:
    """engine.rs:64-85 -- same inputs, same output, computed on the GPU."""
    if not services:
        return []
    p = planner or default_planner()
    perm = p.legacy_order(has_deps_vector(services, flow))
    return [services[i] for i in perm]


def stage_graph(services: list[str], flow: Flow):
    """Target set -> reversed CSR.

    Vertex ids: first occurrence of each name in stage order.  Deps outside the
    target set add no edge (they count as satisfied).  Duplicate deps give
    duplicate edges.  Returns (vertex_names, pos_to_vertex, row_ptr, col, has_deps)."""
    names, pos_to_vertex, row_ptr, col, has_deps = stage_graph_lists(services, flow)
    return (names, np.array(pos_to_vertex, np.uint32), np.array(row_ptr, np.uint32), np.array(col, np.uint32),
            np.frombuffer(has_deps, np.uint8))


def stage_graph_lists(services: list[str], flow: Flow):
    """stage_graph as plain lists (pos_to_vertex, row_ptr, col) and a bytearray (has_deps)."""
    vid: dict[str, int] = {}
    names: list[str] = []
    pos_to_vertex = []
    for n in services:
        if n not in vid:
            vid[n] = len(names)
            names.append(n)
        pos_to_vertex.append(vid[n])
    V = len(names)
    # plain lists, one array conversion each at the end: a fleet.kdl stage has a handful of services,
    # where per-element numpy indexing costs more than the graph (config 1 is timed per plan)
    has_deps = bytearray(V)
    edges = []
    for v, n in enumerate(names):
        svc = flow.services.get(n)
        if svc is None or not svc.depends_on:
            continue
        has_deps[v] = 1
        for d in svc.depends_on:
            u = vid.get(d)
            if u is not None:
                edges.append((u, v))
    row_ptr = [0] * (V + 1)
    for d, _ in edges:
        row_ptr[d + 1] += 1
    for i in range(V):
        row_ptr[i + 1] += row_ptr[i]
    col = [0] * len(edges)
    fill = row_ptr[:-1]
    for d, v in edges:
        col[fill[d]] = v
        fill[d] += 1
    return names, pos_to_vertex, row_ptr, col, has_deps


def levelize_stage(services: list[str], flow: Flow, planner: Planner | None = None):
    """Kahn start levels per position and the (level, position) start order."""
    if not services:
        return [], []
    p = planner or default_planner()
    names, pos2v, row_ptr, col, has_deps = stage_graph(services, flow)
    level_v, _, _ = p.levelize(row_ptr, col, has_deps)
    levels = [int(level_v[v]) for v in pos2v]
    order = sorted(range(len(services)), key=lambda i: (levels[i] == NONE, levels[i], i))
    return levels, [services[i] for i in order]


class LabelDict:
    """Sorted (key=value) dictionary -> bit index, <= 32 labels."""

    def __init__(self, labels):
        self.bits = {lab: i for i, lab in enumerate(sorted(set(labels)))}
        if len(self.bits) > 32:
            raise ValueError("more than 32 distinct labels")

    def mask(self, labels):
        m = 0
        for lab in labels:
            m |= 1 << self.bits[lab]
        return m

    def key_mask(self, key: str) -> int:
        """The bits of every ``key=...`` label of the dictionary: what a fallback hop on ``key`` gives up
        (SPEC.md 2.8).  A key no label uses gives 0."""
        prefix = key + "="
        m = 0
        for lab, bit in self.bits.items():
            if lab.startswith(prefix):
                m |= 1 << bit
        return m


# SPEC.md 2.9: the 2.3 predicates in the bit order of fp_why
WHY_NAMES = ("CORDON", "CPU", "MEM", "LABEL", "CONFLICT")


@dataclass
class Why:
    """Why a service has no server (SPEC.md 2.9, one fp_explain row): per cause the number of servers it
    fails on (``fail``, non-exclusive) and the number where it is the sole blocker (``only``), the servers
    that would still take it (``feasible``; > 0 only for SKEW rejections), the causes that fail on every
    server (``universal``), the required labels no schedulable server carries (``missing_labels``,
    ``key=value``) and the first server one cause away (``nearest``, a slug or None).  ``servers`` is the size of the table the counts are out of."""
    fail: dict[str, int]
    only: dict[str, int]
    feasible: int
    universal: list[str]
    missing_labels: list[str]
    nearest: str | None
    servers: int = 0  # N, the servers of the table the diagnosis was taken on

    @classmethod
    def from_row(cls, row, labels: "LabelDict", slugs: list[str]) -> "Why":
        from ._lib import EXPLAIN_ALL, EXPLAIN_FAIL, EXPLAIN_FEASIBLE, EXPLAIN_MISSING, EXPLAIN_NEAR, EXPLAIN_ONLY
        row = [int(x) for x in row]
        near = row[EXPLAIN_NEAR]
        return cls({n: row[EXPLAIN_FAIL + k] for k, n in enumerate(WHY_NAMES)},
                   {n: row[EXPLAIN_ONLY + k] for k, n in enumerate(WHY_NAMES)}, row[EXPLAIN_FEASIBLE],
                   [n for k, n in enumerate(WHY_NAMES) if row[EXPLAIN_ALL] >> k & 1],
                   [lab for lab, bit in labels.bits.items() if row[EXPLAIN_MISSING] >> bit & 1],
                   slugs[near] if near != NONE else None, len(slugs))


@dataclass
class Plan:
    stage: str
    order: list[str]              # legacy-compatible start order (engine.rs:67-85)
    levels: dict[str, int]        # Kahn levels (U32_MAX = cycle)
    level_order: list[str]        # sort by (level, position)
    assignment: dict[str, str]    # service -> server slug (unplaced absent)
    rejected: dict[str, str]      # service -> "NOFIT" | "CYCLE" | "SKEW" | "QUOTA"
    # stage 2 on the stage's pristine server table: service -> (feasible servers, first feasible
    # slug or None); count 0 is an exact NOFIT before placement (SPEC.md 2.3 monotonicity)
    candidates: dict[str, tuple[int, str | None]] = field(default_factory=dict)
    # the placement strategy the assignment was made under (SPEC.md 2.6); None = first fit
    strategy: str | None = None
    preferred: list[str] = field(default_factory=list)
    # the hard topology spread the assignment was made under (SPEC.md 2.7); None = no constraint
    spread_topology_key: str | None = None
    spread_max_skew: int | None = None
    # the fallback chain the assignment was made under (SPEC.md 2.8); no keys = no fallback.  relaxed:
    # service -> the label keys it required and gave up (services placed at hop >= 1 only)
    fallback_relax_order: list[str] = field(default_factory=list)
    fallback_max_hops: int | None = None
    relaxed: dict[str, list[str]] = field(default_factory=dict)
    # rejection diagnosis (SPEC.md 2.9), plan_stage(..., explain=True): service -> Why for the services
    # rejected NOFIT or SKEW, taken on the server table the placement left; empty otherwise
    why: dict[str, Why] = field(default_factory=dict)
    # the resource quota the assignment was made under (SPEC.md 2.10): the caps (cpu millicores, memory MiB,
    # services; None = no cap in that dimension), the tenant's usage after this plan, and service -> the
    # dimensions that refused it ("cpu", "memory", "services") for the services rejected QUOTA.  None / empty
    # without a quota
    quota: tuple | None = None
    quota_used: tuple | None = None
    quota_why: dict[str, list[str]] = field(default_factory=dict)


def spread_domains(nodes: list[Server], topology_key: str) -> tuple[list[int], list[bool]]:
    """The topology domain of each server under ``topology_key`` (SPEC.md 2.7): the value of its
    ``key=value`` label, numbered in the order of first appearance in node-index order.  A server
    without the key is no candidate under the constraint (k8s PodTopologySpread): has_key is False and
    its domain id is 0, which nothing reads.  More than 64 distinct values is a ValueError."""
    from ._lib import FP_SPREAD_MAX_DOMAINS
    ids: dict[str, int] = {}
    domain, has_key = [], []
    prefix = topology_key + "="
    for nd in nodes:
        value = next((lab[len(prefix):] for lab in nd.labels if lab.startswith(prefix)), None)
        has_key.append(value is not None)
        domain.append(ids.setdefault(value, len(ids)) if value is not None else 0)
    if len(ids) > FP_SPREAD_MAX_DOMAINS:
        raise ValueError(f"spread constraint: topology key '{topology_key}' has {len(ids)} distinct values in this "
                         f"stage (at most {FP_SPREAD_MAX_DOMAINS})")
    return domain, has_key


def _server_nodes(flow: Flow, servers: list[str]):
    out = []
    for s in servers:
        out.append(flow.servers.get(s, Server(slug=s)))
    return out


def _stage_labels(names: list[str], flow: Flow, nodes: list[Server], preferred=()) -> LabelDict:
    """The stage's label dictionary: required, server and (soft) preferred labels."""
    svcs = [flow.services.get(n, Service()) for n in names]
    return LabelDict([lab for s in svcs for lab in s.labels] + [lab for nd in nodes for lab in nd.labels]
                     + list(preferred))


def _stage_tables(names: list[str], flow: Flow, nodes: list[Server], preferred=()):
    """The stage's services (vertex order) and servers as the SoA tables of the C ABI: label,
    host-port and anti-affinity bit dictionaries (SPEC.md 4)."""
    svcs = [flow.services.get(n, Service()) for n in names]
    ld = _stage_labels(names, flow, nodes, preferred)
    ports = sorted({hp for s in svcs for hp in s.host_ports})
    groups = sorted({s.anti_affinity for s in svcs if s.anti_affinity})
    if len(ports) > 16 or len(groups) > 16:
        raise ValueError("more than 16 host ports or anti-affinity groups in one stage")
    pbit = {hp: i for i, hp in enumerate(ports)}
    gbit = {g: 16 + i for i, g in enumerate(groups)}
    cpu = [s.cpu_m for s in svcs]
    mem = [s.mem_mib for s in svcs]
    req = [ld.mask(s.labels) for s in svcs]
    conf = []
    for s in svcs:
        m = 0
        for hp in s.host_ports:
            m |= 1 << pbit[hp]
        if s.anti_affinity:
            m |= 1 << gbit[s.anti_affinity]
        conf.append(m)
    cf = [nd.cpu_m for nd in nodes]
    mf = [nd.mem_mib for nd in nodes]
    lab = [ld.mask(nd.labels) for nd in nodes]
    cu = [0] * len(nodes)
    sch = [1 if nd.schedulable else 0 for nd in nodes]
    return (cpu, mem, req, conf), (cf, mf, lab, cu, sch)


def plan_stage(flow: Flow, stage_name: str, planner: Planner | None = None,
               servers: list[Server] | None = None, policy: PlacementPolicy | None = None,
               explain: bool = False, quota_used=(0, 0, 0)) -> Plan:
    """Full planner output for one stage (SPEC.md 2): the `fleet up --dry-run`
    plan (up.rs:57-136).  One fp_plan_stage call -- A1 order, A2 levels, and with servers the stage-2
    candidates and the FFD plan -- when every service name appears once in the stage; a stage
    listing a name twice (positions != vertices) takes the per-output calls.

    ``policy`` (or, without one, the stage's parsed ``placement`` node) selects a placement strategy,
    soft preferred labels (SPEC.md 2.6), a hard topology spread (SPEC.md 2.7) and a fallback chain
    (SPEC.md 2.8): levels, orders and candidates are computed as without one, and the assignment comes
    from ``Planner.place_policy``, or ``Planner.place_policy_fallback`` when the policy has a chain.
    Under a chain each hop gives up every ``key=...`` label of one key (``LabelDict.key_mask`` over the
    stage's dictionary); ``Plan.relaxed`` names, per service placed at hop >= 1, the keys it required
    and gave up.
    Under a spread constraint the servers' ``topology_key=value`` labels give the domains
    (``spread_domains``); a server without the key goes to the policy call as unschedulable and
    receives nothing, and a service some server fits but none within the skew is rejected as "SKEW".
    Under a resource quota (SPEC.md 2.10; ``policy.quota``) the assignment comes from
    ``Planner.place_policy_quota``: ``quota_used`` = (cpu millicores, memory MiB, services) is what the
    tenant holds already, a service the quota refuses is rejected as "QUOTA" before any server is tried,
    ``Plan.quota_why`` names the dimensions that refused it, and ``Plan.quota`` / ``Plan.quota_used`` carry
    the caps and the usage after the plan.  A stage without servers places nothing and is planned as
    without a quota.
    No policy, or one that sets nothing: exactly the path above.

    ``explain=True`` adds the rejection diagnosis of SPEC.md 2.9: ``Plan.why[name]`` for every service
    rejected NOFIT or SKEW, one ``Planner.explain`` call on the server table the placement left (the table
    the placer was given: under a spread constraint the servers without the topology key are
    unschedulable there), with the label bits of the fallback chain's keys given up.  The default changes
    nothing: ``Plan.why`` stays empty."""
    p = planner or default_planner()
    stage = flow.stages[stage_name]
    services = list(stage.services)
    nodes = servers if servers is not None else _server_nodes(flow, stage.servers)
    pol = policy if policy is not None else stage.placement
    if pol is not None and not pol.active:
        pol = None
    assignment, rejected, candidates, relaxed = {}, {}, {}, {}
    quota_after, quota_why = None, {}
    ignore = 0  # SPEC.md 2.9: the label bits a fallback chain gives up
    if not services:
        return Plan(stage_name, [], {}, [], assignment, rejected, candidates)
    if not nodes:
        # no servers (the fleet.kdl fixtures): the graph stays in lists, one prebuilt call
        names, pos2v, row_ptr, col, has_deps = stage_graph_lists(services, flow)
        if len(names) == len(services):
            perm, levels, order_v, _ = p.plan_stage_lists(row_ptr, col, has_deps)
            return Plan(stage_name, [services[i] for i in perm], dict(zip(services, levels)),
                        [services[i] for i in order_v], assignment, rejected, candidates)
    names, pos2v, row_ptr, col, has_deps = stage_graph(services, flow)
    if len(names) == len(services):
        cont, ntab = _stage_tables(names, flow, nodes) if nodes else (None, None)
        perm, level_v, order_v, _, placed = p.plan_stage(row_ptr, col, has_deps, cont, ntab)
        order = [services[i] for i in perm.tolist()]
        levels = level_v.tolist()
        level_order = [services[i] for i in order_v.tolist()]
    else:
        order = order_by_dependencies(services, flow, p)
        levels, level_order = levelize_stage(services, flow, p)
        placed = None
        if nodes:
            lvl_v = {names[v]: levels[i] for i, v in enumerate(pos2v)}
            cont, ntab = _stage_tables(names, flow, nodes)
            # stage 2 (fp_feasibility): feasible-server count and first feasible server per service
            first, count, _ = p.feasibility(cont, ntab, bitmap=False)
            assign, reason, after = p.place(cont, ntab, level=[lvl_v[n] for n in names])
            placed = (first, count, assign, reason, after)
    if placed is not None and pol is not None:
        # the scored placer on the same tables; the preferred labels share the stage's dictionary
        lvl_v = dict(zip(services, levels))
        cont, ntab = _stage_tables(names, flow, nodes, pol.preferred)
        pmask = _stage_labels(names, flow, nodes, pol.preferred).mask(pol.preferred)
        domain, max_skew = None, 0
        if pol.spread is not None:
            domain, has_key = spread_domains(nodes, pol.spread[0])
            max_skew = pol.spread[1]
            ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
        strategy = pol.strategy if pol.strategy is not None else 0
        if pol.fallback or pol.quota is not None:
            ld = _stage_labels(names, flow, nodes, pol.preferred)
            relax = [ld.key_mask(k) for k in pol.fallback]
            if pol.quota is not None:
                from ._lib import QUOTA_NAMES
                assign, reason, hops, after, _, qwhy, qused = p.place_policy_quota(
                    cont, ntab, strategy, pol.quota, quota_used, relax, preferred=pmask,
                    level=[lvl_v[n] for n in names], domain=domain, max_skew=max_skew)
                quota_after = tuple(int(x) for x in qused)
                quota_why = {n: [d for k, d in enumerate(QUOTA_NAMES) if qwhy[v] >> k & 1]
                             for v, n in enumerate(names) if reason[v] == 4}
            else:
                assign, reason, hops, after, _ = p.place_policy_fallback(cont, ntab, strategy, relax, preferred=pmask,
                                                                         level=[lvl_v[n] for n in names], domain=domain,
                                                                         max_skew=max_skew)
            for m in relax:
                ignore |= m
            for v, n in enumerate(names):
                if assign[v] != NONE and hops[v]:
                    required = {lab.split("=", 1)[0] for lab in flow.services.get(n, Service()).labels}
                    relaxed[n] = [k for k in pol.fallback[:int(hops[v])] if k in required]
        else:
            assign, reason, after, _ = p.place_policy(cont, ntab, strategy, preferred=pmask, level=[lvl_v[n] for n in names],
                                                      domain=domain, max_skew=max_skew)
        placed = (placed[0], placed[1], assign, reason, after)
    why = {}
    if placed is not None:
        first, count, assign, reason, after = placed
        candidates = {n: (int(count[v]), nodes[int(first[v])].slug if int(first[v]) != NONE else None)
                      for v, n in enumerate(names)}
        for v, n in enumerate(names):
            if assign[v] != NONE:
                assignment[n] = nodes[assign[v]].slug
            else:
                rejected[n] = {2: "CYCLE", 3: "SKEW", 4: "QUOTA"}.get(int(reason[v]), "NOFIT")
        sel = [v for v, n in enumerate(names) if rejected.get(n) in ("NOFIT", "SKEW")]
        if explain and sel:
            # cont holds the tables of the call that made the assignment, `after` the server table it left
            rows = p.explain(cont, after, sel=sel, ignore_labels=ignore)
            ld = _stage_labels(names, flow, nodes, pol.preferred if pol is not None else ())
            slugs = [nd.slug for nd in nodes]
            why = {names[v]: Why.from_row(rows[i], ld, slugs) for i, v in enumerate(sel)}
    plan = Plan(stage_name, order, dict(zip(services, levels)), level_order, assignment, rejected, candidates)
    plan.why = why
    if placed is not None and pol is not None:
        plan.strategy, plan.preferred = pol.strategy, pol.preferred
        if pol.spread is not None:
            plan.spread_topology_key, plan.spread_max_skew = pol.spread
        if pol.fallback:
            plan.fallback_relax_order, plan.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
            plan.relaxed = relaxed
        if pol.quota is not None:
            plan.quota, plan.quota_used, plan.quota_why = pol.quota, quota_after, quota_why
    return plan


@dataclass
class DrainCandidate:
    """One candidate of a drain sweep (SPEC.md 2.11): the servers taken out together, where their services
    go and which are left without a server."""
    name: str                              # the server's slug, "key=value" of a topology domain, or slugs joined by ","
    servers: list[str]                     # the candidate's servers (slugs, node order)
    moves: list[tuple[str, str, str]]      # (service, from, to) in visiting order (cpu desc, mem desc, stage order)
    stranded: list[str]                    # services no remaining server takes, in visiting order
    evicted: int = 0                       # services running on the candidate
    stranded_cpu_m: int = 0                # what the stranded services ask for in sum
    stranded_mem_mib: int = 0
    targets: int = 0                       # distinct servers that receive a service
    # under the policy (SPEC.md 2.15, drain_stage(under_policy=True)); unset otherwise
    relaxed: dict[str, list[str]] = field(default_factory=dict)   # moved service -> label keys given up (Plan.relaxed)
    stranded_reason: dict[str, str] = field(default_factory=dict)  # stranded service -> "NOFIT" / "SKEW"
    skew_before: int | None = None         # max - min of the services per eligible domain without the candidate
    skew_after: int | None = None          # the same after its moves


@dataclass
class DrainReport:
    """``drain_stage``'s answer: one DrainCandidate per candidate, every one computed independently from the
    same live state, under the strategy and preferred labels named here, and with ``under_policy`` under the
    spread constraint and the fallback chain named here."""
    stage: str
    by: str | None = None                  # the topology key the candidates are the values of; None = servers
    strategy: str | None = None
    preferred: list[str] = field(default_factory=list)
    candidates: list[DrainCandidate] = field(default_factory=list)
    # the guarantees the moves were held to (SPEC.md 2.15); unset without under_policy
    spread_topology_key: str | None = None
    spread_max_skew: int | None = None
    fallback_relax_order: list[str] = field(default_factory=list)
    fallback_max_hops: int | None = None


def live_tables(flow: Flow, stage_name: str, plan: Plan, policy: PlacementPolicy | None = None):
    """The live state ``plan`` describes, as the inputs of a drain sweep (SPEC.md 2.11): the stage's tables
    rebuilt as ``plan_stage`` builds them, with every assigned service's request deducted on its server.
    Returns (names, nodes, cont, live, assign, node_count, strategy, preferred_mask): ``live`` = (cpu_free,
    mem_free, labels, conflict_used, schedulable) lists, ``assign[v]`` the node index of service ``names[v]``
    or NONE, ``node_count[n]`` the services on server n.  Strategy and preferred labels are ``policy``'s, or
    without one those the plan was made under.  A plan that names a server the stage does not have is a
    ValueError."""
    stage = flow.stages[stage_name]
    names = list(dict.fromkeys(stage.services))
    nodes = _server_nodes(flow, stage.servers)
    strategy = policy.strategy if policy is not None else plan.strategy
    preferred = policy.preferred if policy is not None else list(plan.preferred)
    cont, (cf, mf, lab, cu, sch) = _stage_tables(names, flow, nodes, preferred)
    pmask = _stage_labels(names, flow, nodes, preferred).mask(preferred)
    index = {nd.slug: n for n, nd in enumerate(nodes)}
    assign, count = [NONE] * len(names), [0] * len(nodes)
    for v, name in enumerate(names):
        slug = plan.assignment.get(name)
        if slug is None:
            continue
        if slug not in index:
            raise ValueError(f"plan for stage '{stage_name}' runs '{name}' on '{slug}', which is no server of the stage")
        n = index[slug]
        assign[v] = n
        cf[n] = (cf[n] - cont[0][v]) & U32_MAX
        mf[n] = (mf[n] - cont[1][v]) & U32_MAX
        cu[n] |= cont[3][v]
        count[n] += 1
    return names, nodes, cont, (cf, mf, lab, cu, sch), assign, count, strategy, pmask


def drain_stage(flow: Flow, stage_name: str, plan: Plan, by: str | None = None, servers: list[str] | None = None,
                planner: Planner | None = None, policy: PlacementPolicy | None = None,
                under_policy: bool = False) -> DrainReport:
    """"Can this server, or this whole zone, be taken out?" for a stage that runs as ``plan`` says (SPEC.md
    2.11; the `drain` scheduling state of model.rs:435-442): one ``Planner.drain_sweep`` over the live
    tables of ``live_tables``.  The candidates are

    * ``servers=[slugs]``: those servers together, one candidate;
    * ``by="region"`` (any topology key): one candidate per value of the key among the stage's servers
      (``spread_domains``; a server without the key belongs to none);
    * neither: the servers flagged ``draining`` together when the stage has any (what the registry says is
      leaving), otherwise each server on its own.

    Every candidate is computed independently from the same live state: its services are visited in the
    order (cpu desc, mem desc, stage order) and go to the remaining schedulable servers under the strategy
    and preferred labels of ``policy`` or, without one, of the policy the plan was made under.  By default
    the policy's spread constraint and fallback chain are not applied to moves: a move is a SPEC.md 2.6
    placement.

    ``under_policy=True`` applies them (SPEC.md 2.15, one ``Planner.drain_sweep_policy`` call): the spread
    constraint and the chain of ``policy`` or, without one, of the policy the plan was made under.  Each
    candidate's domain counts leave its own servers out, a domain counts while it keeps a target, and servers
    without the topology key take no move (``replan_domains``).  A quota has nothing to test: a move releases
    and retakes the same request.  The candidates then carry ``relaxed``, ``stranded_reason``, ``skew_before``
    and ``skew_after``, and the report the guarantees it ran under."""
    p = planner or default_planner()
    names, nodes, cont, live, assign, count, strategy, pmask = live_tables(flow, stage_name, plan, policy)
    pol_pref = policy.preferred if policy is not None else list(plan.preferred)
    report = DrainReport(stage_name, None, strategy, pol_pref)
    pol = None
    if under_policy:
        pol = policy if policy is not None else _plan_policy(plan)
        if pol.spread is not None:
            report.spread_topology_key, report.spread_max_skew = pol.spread
        if pol.fallback:
            report.fallback_relax_order, report.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    if not nodes:
        return report
    slugs = [nd.slug for nd in nodes]
    if servers is None and by is None and any(nd.draining for nd in nodes):
        servers = [nd.slug for nd in nodes if nd.draining]
    if servers is not None:
        unknown = [s for s in servers if s not in slugs]
        if unknown:
            raise ValueError(f"drain: {unknown} are no servers of stage '{stage_name}'")
        chosen = set(servers)
        group = [0 if s in chosen else NONE for s in slugs]
        cand_names = [",".join(s for s in slugs if s in chosen)]
    elif by is not None:
        report.by = by
        domain, has_key = spread_domains(nodes, by)
        group = [d if k else NONE for d, k in zip(domain, has_key)]
        cand_names = [""] * (max((g for g in group if g != NONE), default=-1) + 1)
        prefix = by + "="
        for nd, g in zip(nodes, group):
            if g != NONE and not cand_names[g]:
                cand_names[g] = next(lab for lab in nd.labels if lab.startswith(prefix))
    else:
        group = list(range(len(nodes)))
        cand_names = slugs
    n_cand = len(cand_names)
    from ._lib import (DRAIN_EVICTED, DRAIN_SKEW_AFTER, DRAIN_SKEW_BEFORE, DRAIN_STRANDED_CPU, DRAIN_STRANDED_MEM,
                       DRAIN_TARGETS, REASON_SKEW)
    reason = hops = rows = None
    if pol is None:
        out, _, summary = p.drain_sweep(cont, live, assign, group, n_cand, strategy if strategy is not None else 0,
                                        pmask, count)
    else:
        domain, max_skew = None, 0
        if pol.spread is not None:
            domain, has_key = replan_domains(nodes, pol.spread[0])
            max_skew = pol.spread[1]
            live = (*live[:4], [s if k else 0 for s, k in zip(live[4], has_key)])
        relax = [_stage_labels(names, flow, nodes, pol_pref).key_mask(k) for k in pol.fallback]
        out, reason, summary, hops, rows = p.drain_sweep_policy(
            cont, live, assign, group, n_cand, strategy if strategy is not None else 0, pmask, count, domain=domain,
            max_skew=max_skew, relax_mask=relax)
    evictees: list[list[int]] = [[] for _ in range(n_cand)]
    for v, n in enumerate(assign):
        if n != NONE and group[n] != NONE:
            evictees[group[n]].append(v)
    for k, name in enumerate(cand_names):
        evictees[k].sort(key=lambda v: (-cont[0][v], -cont[1][v], v))  # the visiting order
        moves = [(names[v], slugs[assign[v]], slugs[int(out[v])]) for v in evictees[k] if int(out[v]) != NONE]
        stranded = [names[v] for v in evictees[k] if int(out[v]) == NONE]
        row = [int(x) for x in summary[k]]
        cand = DrainCandidate(name, [s for s, g in zip(slugs, group) if g == k], moves, stranded,
                              row[DRAIN_EVICTED], row[DRAIN_STRANDED_CPU], row[DRAIN_STRANDED_MEM], row[DRAIN_TARGETS])
        if pol is not None:
            for v in evictees[k]:
                if int(out[v]) == NONE:
                    cand.stranded_reason[names[v]] = "SKEW" if int(reason[v]) == REASON_SKEW else "NOFIT"
                elif int(hops[v]):
                    required = {lab.split("=", 1)[0] for lab in flow.services.get(names[v], Service()).labels}
                    cand.relaxed[names[v]] = [key for key in pol.fallback[:int(hops[v])] if key in required]
            if pol.spread is not None:
                cand.skew_before, cand.skew_after = int(rows[k][DRAIN_SKEW_BEFORE]), int(rows[k][DRAIN_SKEW_AFTER])
        report.candidates.append(cand)
    return report


@dataclass
class ShrinkVariant:
    """One release order of a scale-in sweep (SPEC.md 2.16): the servers it gives back, what moves so that it
    can, and the servers it tried and could not free."""
    name: str                              # the rule's name, or "order<i>" for an explicit list
    order: list[str]                       # the servers in the order they were tried (slugs)
    released: list[str]                    # the servers given back, in try order
    moves: list[tuple[str, str, str]]      # (service, from, to): from = the server of the base plan, to = the final one
    stayed: list[tuple[str, str]]          # (server, blocker service) for each server whose last attempt failed
    tried: int = 0                         # attempts made
    failed: int = 0                        # attempts undone
    n_moves: int = 0                       # committed moves; a service that moved twice counts twice
    moved_cpu_m: int = 0                   # what the moved services ask for in sum
    moved_mem_mib: int = 0
    # under the policy (SPEC.md 2.17, shrink_stage(under_policy=True)); unset otherwise.  A server the bound rule
    # kept has no blocker service: its ``stayed`` entry is (server, None)
    relaxed: dict[str, list[str]] = field(default_factory=dict)  # moved service -> label keys given up (Plan.relaxed)
    stayed_reason: dict[str, str] = field(default_factory=dict)  # server that stayed -> "NOFIT" / "SKEW" / "BOUND"
    skew_before: int | None = None         # max - min of the services per eligible domain on the live state
    skew_after: int | None = None          # the same on the state the variant leaves


@dataclass
class ShrinkReport:
    """``shrink_stage``'s answer: one ShrinkVariant per release order, every one computed independently from the
    same live state under the strategy and preferred labels named here, and with ``under_policy`` under the
    spread constraint and the fallback chain named here.  ``best`` indexes the variant with the
    most released servers, then the fewest moved services, then the lowest index (None without variants), and
    ``plan`` is the plan that variant leaves."""
    stage: str
    strategy: str | None = None
    preferred: list[str] = field(default_factory=list)
    keep: list[str] = field(default_factory=list)
    variants: list[ShrinkVariant] = field(default_factory=list)
    best: int | None = None
    plan: Plan | None = None
    # the guarantees the moves were held to (SPEC.md 2.17); unset without under_policy
    spread_topology_key: str | None = None
    spread_max_skew: int | None = None
    fallback_relax_order: list[str] = field(default_factory=list)
    fallback_max_hops: int | None = None


SHRINK_RULES = ("fewest", "lightest", "last")


def shrink_order(rule: str, nodes: list[Server], cont, assign, keep=()) -> list[int]:
    """The node indices a rule tries, in order: the servers flagged ``draining`` first, then ``"fewest"`` by
    running services ascending, ``"lightest"`` by the sum of the running cpu requests ascending, ``"last"`` by
    node order descending (the reverse of the way first fit fills); ties in node order.  ``keep`` (slugs) are
    left out."""
    if rule not in SHRINK_RULES:
        raise ValueError(f"shrink: unknown order rule '{rule}' (one of {', '.join(SHRINK_RULES)})")
    count, load = [0] * len(nodes), [0] * len(nodes)
    for v, n in enumerate(assign):
        if n != NONE:
            count[n] += 1
            load[n] += cont[0][v]
    held = set(keep)
    idx = [n for n, nd in enumerate(nodes) if nd.slug not in held]
    if rule == "fewest":
        key = lambda n: (not nodes[n].draining, count[n], n)  # noqa: E731
    elif rule == "lightest":
        key = lambda n: (not nodes[n].draining, load[n], n)  # noqa: E731
    else:
        key = lambda n: (not nodes[n].draining, -n)  # noqa: E731
    return sorted(idx, key=key)


def shrink_stage(flow: Flow, stage_name: str, plan: Plan, orders=None, keep=None, planner: Planner | None = None,
                 policy: PlacementPolicy | None = None, under_policy: bool = False) -> ShrinkReport:
    """"Which servers can I hand back, and what has to move so that I can?" for a stage that runs as ``plan``
    says (SPEC.md 2.16): one ``Planner.shrink_sweep`` over the live tables of ``live_tables``, one variant per
    entry of ``orders``.  An entry is a rule name (``shrink_order``: "fewest", "lightest", "last") or an explicit
    list of server slugs; the default is all three rules.  ``keep`` (slugs) are never tried, in a rule or in an
    explicit list; an unknown slug anywhere is a ValueError.

    A variant tries its servers one after the other on the state its earlier releases left: the server's
    services are visited in the order (cpu desc, mem desc, stage order) and go to the remaining schedulable
    servers under the strategy and preferred labels of ``policy`` or, without one, of the policy the plan was
    made under; if one of them finds no server the attempt is undone and the server stays.  By default the
    policy's spread constraint and fallback chain are not applied to moves: a move is a SPEC.md 2.6 placement.

    ``under_policy=True`` applies them (SPEC.md 2.17, one ``Planner.shrink_sweep_policy`` call): the spread
    constraint and the chain of ``policy`` or, without one, of the policy the plan was made under.  The domain
    counts leave the released servers and the tried one out, a domain counts while it keeps a target, servers
    without the topology key take no move (``replan_domains``), and a release that would take the stage out of
    ``max_skew``, or further out, is refused although every move passed (the bound rule).  A quota has nothing
    to test: a move releases and retakes the same request.  The variants then carry ``relaxed``,
    ``stayed_reason``, ``skew_before`` and ``skew_after``, the report the guarantees it ran under, and the best
    order's plan ``relaxed`` for the services it moved."""
    import dataclasses
    from ._lib import (REASON_SKEW, SHRINK_FAILED, SHRINK_MOVED_CPU, SHRINK_MOVED_MEM, SHRINK_MOVES, SHRINK_SKEW_AFTER,
                       SHRINK_SKEW_BEFORE, SHRINK_STATE_FAILED, SHRINK_STATE_RELEASED, SHRINK_TRIED)
    p = planner or default_planner()
    names, nodes, cont, live, assign, count, strategy, pmask = live_tables(flow, stage_name, plan, policy)
    pol_pref = policy.preferred if policy is not None else list(plan.preferred)
    keep = list(keep or [])
    report = ShrinkReport(stage_name, strategy, pol_pref, keep)
    pol = None
    if under_policy:
        pol = policy if policy is not None else _plan_policy(plan)
        if pol.spread is not None:
            report.spread_topology_key, report.spread_max_skew = pol.spread
        if pol.fallback:
            report.fallback_relax_order, report.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    slugs = [nd.slug for nd in nodes]
    index = {s: n for n, s in enumerate(slugs)}
    unknown = [s for s in keep if s not in index]
    if unknown:
        raise ValueError(f"shrink: {unknown} are no servers of stage '{stage_name}'")
    rows, labels = [], []
    for i, entry in enumerate(SHRINK_RULES if orders is None else orders):
        if isinstance(entry, str):
            rows.append(shrink_order(entry, nodes, cont, assign, keep))
            labels.append(entry)
        else:
            unknown = [s for s in entry if s not in index]
            if unknown:
                raise ValueError(f"shrink: {unknown} are no servers of stage '{stage_name}'")
            rows.append([index[s] for s in entry if s not in keep])
            labels.append(f"order{i}")
    if not rows:
        return report
    n_try = max(len(r) for r in rows)
    try_order = np.full((len(rows), n_try), NONE, np.uint32)
    for i, r in enumerate(rows):
        try_order[i, :len(r)] = r
    hops = why = prows = None
    if pol is None:
        out, state, blocker, summary = p.shrink_sweep(cont, live, assign, try_order,
                                                      strategy if strategy is not None else 0, pmask, count)
    else:
        domain, max_skew = None, 0
        if pol.spread is not None:
            domain, has_key = replan_domains(nodes, pol.spread[0])
            max_skew = pol.spread[1]
            live = (*live[:4], [s if k else 0 for s, k in zip(live[4], has_key)])
        relax = [_stage_labels(names, flow, nodes, pol_pref).key_mask(k) for k in pol.fallback]
        out, state, blocker, summary, hops, why, prows = p.shrink_sweep_policy(
            cont, live, assign, try_order, strategy if strategy is not None else 0, pmask, count, domain=domain,
            max_skew=max_skew, relax_mask=relax)
    visit = sorted(range(len(names)), key=lambda v: (-cont[0][v], -cont[1][v], v))
    for i, r in enumerate(rows):
        row = [int(x) for x in summary[i]]
        freed = [slugs[n] for n in dict.fromkeys(r) if int(state[i][n]) == SHRINK_STATE_RELEASED]
        moves = [(names[v], slugs[assign[v]], slugs[int(out[i][v])]) for v in visit if int(out[i][v]) != assign[v]]
        held = [n for n in dict.fromkeys(r) if int(state[i][n]) == SHRINK_STATE_FAILED]
        stayed = [(slugs[n], names[int(blocker[i][n])] if int(blocker[i][n]) != NONE else None) for n in held]
        var = ShrinkVariant(labels[i], [slugs[n] for n in r], freed, moves, stayed, row[SHRINK_TRIED],
                            row[SHRINK_FAILED], row[SHRINK_MOVES], row[SHRINK_MOVED_CPU], row[SHRINK_MOVED_MEM])
        if pol is not None:
            for n in held:
                var.stayed_reason[slugs[n]] = ("BOUND" if int(blocker[i][n]) == NONE
                                               else "SKEW" if int(why[i][n]) == REASON_SKEW else "NOFIT")
            for v in visit:
                if int(out[i][v]) != assign[v] and int(hops[i][v]):
                    required = {lab.split("=", 1)[0] for lab in flow.services.get(names[v], Service()).labels}
                    var.relaxed[names[v]] = [key for key in pol.fallback[:int(hops[i][v])] if key in required]
            if pol.spread is not None:
                var.skew_before, var.skew_after = int(prows[i][SHRINK_SKEW_BEFORE]), int(prows[i][SHRINK_SKEW_AFTER])
        report.variants.append(var)
    report.best = min(range(len(rows)), key=lambda i: (-len(report.variants[i].released), len(report.variants[i].moves), i))
    best = report.variants[report.best]
    assignment = dict(plan.assignment)
    for svc, _, dst in best.moves:
        assignment[svc] = dst
    report.plan = dataclasses.replace(plan, assignment=assignment)
    if pol is not None:  # a moved service carries the keys its last move gave up, and no others
        relaxed = {svc: keys for svc, keys in plan.relaxed.items() if svc not in {m[0] for m in best.moves}}
        relaxed.update(best.relaxed)
        report.plan = dataclasses.replace(report.plan, relaxed=relaxed)
    return report


@dataclass
class RebalanceVariant:
    """One victim order of a rebalance sweep (SPEC.md 2.19): the seats it gives up to bring the spread constraint
    back within ``max_skew``, where they go, and the services it tried and could not move."""
    name: str                              # the rule's name, or "order<i>" for an explicit list
    order: list[str]                       # the services in the order they were visited
    moves: list[tuple[str, str, str]]      # (service, from, to), in victim order
    stuck: dict[str, str] = field(default_factory=dict)          # service whose last attempt failed -> "NOFIT" / "SKEW"
    relaxed: dict[str, list[str]] = field(default_factory=dict)  # moved service -> label keys given up (Plan.relaxed)
    n_stuck: int = 0                       # rejected attempts; a service tried twice counts twice
    max_moves: int | None = None           # the move budget; None = unlimited
    moved_cpu_m: int = 0                   # what the moved services ask for in sum
    moved_mem_mib: int = 0
    skew_before: int = 0                   # max - min of the services per eligible domain on the live state
    skew_after: int = 0                    # the same on the state the variant leaves
    lightest: str | None = None            # where skew_after is out of bound: the eligible "key=value" with the fewest


@dataclass
class RebalanceReport:
    """``rebalance_stage``'s answer: one RebalanceVariant per victim order, every one computed independently from
    the same live state under the strategy, preferred labels, spread constraint and fallback chain named here.
    ``best`` indexes the variant that ends within ``max_skew`` if one does, then the one with the smallest
    ``skew_after``, the fewest moves, the least moved CPU and the lowest index (None without variants); ``plan`` is
    the plan that variant leaves.  ``note`` says why a report has no variants."""
    stage: str
    strategy: str | None = None
    preferred: list[str] = field(default_factory=list)
    pin: list[str] = field(default_factory=list)
    variants: list[RebalanceVariant] = field(default_factory=list)
    best: int | None = None
    plan: Plan | None = None
    spread_topology_key: str | None = None
    spread_max_skew: int | None = None
    fallback_relax_order: list[str] = field(default_factory=list)
    fallback_max_hops: int | None = None
    note: str | None = None


REBALANCE_RULES = ("smallest", "largest", "newest")


def rebalance_order(rule: str, names: list[str], cont, assign, pin=()) -> list[int]:
    """The service indices a rule visits, in order: ``"smallest"`` by (cpu asc, mem asc, stage order), ``"largest"``
    in the order of SPEC.md 2.3 (cpu desc, mem desc, stage order), ``"newest"`` by stage order descending.  Only
    services that run are listed; ``pin`` (names) are left out."""
    if rule not in REBALANCE_RULES:
        raise ValueError(f"rebalance: unknown order rule '{rule}' (one of {', '.join(REBALANCE_RULES)})")
    held = set(pin)
    idx = [v for v, n in enumerate(names) if n not in held and assign[v] != NONE]
    if rule == "smallest":
        key = lambda v: (cont[0][v], cont[1][v], v)  # noqa: E731
    elif rule == "largest":
        key = lambda v: (-cont[0][v], -cont[1][v], v)  # noqa: E731
    else:
        key = lambda v: -v  # noqa: E731
    return sorted(idx, key=key)


def rebalance_stage(flow: Flow, stage_name: str, plan: Plan, orders=None, pin=None, max_moves=None,
                    policy: PlacementPolicy | None = None, planner: Planner | None = None) -> RebalanceReport:
    """"Which services have to move so that the spread holds again?" for a stage that runs as ``plan`` says (SPEC.md
    2.19; the descheduler to ``replan_stage``'s scheduler): one ``Planner.rebalance_sweep`` over the live tables of
    ``live_tables``, one variant per entry of ``orders``.  An entry is a rule name (``rebalance_order``: "smallest",
    "largest", "newest") or an explicit list of service names; the default is all three rules.  ``pin`` (names) are
    never victims, in a rule or in an explicit list; an unknown name anywhere is a ValueError.  ``max_moves`` is the
    move budget of every variant, or one per variant (None = unlimited).

    A variant visits its services in order.  One that runs in a heavy domain (a value of the topology key that holds
    more than ``max_skew`` services above the lightest eligible one) is lifted off its server and placed again under
    the strategy, preferred labels, spread constraint and fallback chain of ``policy`` or, without one, of the
    policy the plan was made under; if no server takes it, it stays where it was.  Servers without the topology key
    take no move, but what runs on them counts (``replan_domains``).  A rule visits its order twice, so that a
    service that was refused is tried again on the state the others left.  A quota has nothing to test: a move
    releases and retakes the same request.

    A stage without a spread constraint has nothing to restore: the report has no variants and ``note`` says so."""
    import dataclasses
    from ._lib import (REASON_SKEW, REBAL_MOVED_CPU, REBAL_MOVED_MEM, REBAL_SKEW_AFTER, REBAL_SKEW_BEFORE, REBAL_STUCK)
    pol = policy if policy is not None else _plan_policy(plan)
    names, nodes, cont, live, assign, count, strategy, pmask = live_tables(flow, stage_name, plan, policy)
    pin = list(pin or [])
    report = RebalanceReport(stage_name, strategy, list(pol.preferred), pin)
    if pol.fallback:
        report.fallback_relax_order, report.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    index = {n: v for v, n in enumerate(names)}
    unknown = [s for s in pin if s not in index]
    if unknown:
        raise ValueError(f"rebalance: {unknown} are no services of stage '{stage_name}'")
    rows, labels = [], []
    for i, entry in enumerate(REBALANCE_RULES if orders is None else orders):
        if isinstance(entry, str):
            rows.append(rebalance_order(entry, names, cont, assign, pin) * 2)
            labels.append(entry)
        else:
            unknown = [s for s in entry if s not in index]
            if unknown:
                raise ValueError(f"rebalance: {unknown} are no services of stage '{stage_name}'")
            rows.append([index[s] for s in entry if s not in pin])
            labels.append(f"order{i}")
    if pol.spread is None or not pol.spread[1]:
        report.note = "no spread constraint: nothing to restore"
        return report
    report.spread_topology_key, report.spread_max_skew = pol.spread
    if not rows or not nodes:
        report.note = "no victim orders" if not rows else "no servers"
        return report
    budgets = None
    if max_moves is not None:
        per = list(max_moves) if isinstance(max_moves, (list, tuple)) else [max_moves] * len(rows)
        if len(per) != len(rows):
            raise ValueError("rebalance: max_moves must hold one budget per order")
        budgets = [NONE if b is None else int(b) for b in per]
    key, max_skew = pol.spread
    domain, has_key = replan_domains(nodes, key)
    live = (*live[:4], [s if k else 0 for s, k in zip(live[4], has_key)])
    relax = [_stage_labels(names, flow, nodes, list(pol.preferred)).key_mask(k) for k in pol.fallback]
    n_try = max(len(r) for r in rows)
    victim_order = np.full((len(rows), n_try), NONE, np.uint32)
    for i, r in enumerate(rows):
        victim_order[i, :len(r)] = r
    p = planner or default_planner()
    out, hops, why, summary = p.rebalance_sweep(cont, live, assign, victim_order, strategy if strategy is not None else 0,
                                                pmask, count, domain=domain, max_skew=max_skew, relax_mask=relax,
                                                max_moves=budgets)
    slugs = [nd.slug for nd in nodes]
    prefix = key + "="
    value = {}
    for nd, d, k in zip(nodes, domain, has_key):
        if k:
            value.setdefault(d, next(lab for lab in nd.labels if lab.startswith(prefix)))
    eligible = sorted({d for d, s in zip(domain, live[4]) if s})
    for i, r in enumerate(rows):
        row = [int(x) for x in summary[i]]
        seen = list(dict.fromkeys(r))
        moves = [(names[v], slugs[assign[v]], slugs[int(out[i][v])]) for v in seen if int(out[i][v]) != assign[v]]
        var = RebalanceVariant(labels[i], [names[v] for v in r], moves, n_stuck=row[REBAL_STUCK],
                               max_moves=None if budgets is None or budgets[i] == NONE else budgets[i],
                               moved_cpu_m=row[REBAL_MOVED_CPU], moved_mem_mib=row[REBAL_MOVED_MEM],
                               skew_before=row[REBAL_SKEW_BEFORE], skew_after=row[REBAL_SKEW_AFTER])
        for v in seen:
            if int(why[i][v]):
                var.stuck[names[v]] = "SKEW" if int(why[i][v]) == REASON_SKEW else "NOFIT"
            if int(out[i][v]) != assign[v] and int(hops[i][v]):
                required = {lab.split("=", 1)[0] for lab in flow.services.get(names[v], Service()).labels}
                var.relaxed[names[v]] = [k for k in pol.fallback[:int(hops[i][v])] if k in required]
        if var.skew_after > max_skew and eligible:
            per = dict.fromkeys(eligible, 0)
            for v, n in enumerate(out[i]):
                if int(n) != NONE and domain[int(n)] in per:
                    per[domain[int(n)]] += 1
            var.lightest = value[min(eligible, key=lambda d: (per[d], d))]
        report.variants.append(var)
    vs = report.variants
    report.best = min(range(len(vs)), key=lambda i: (vs[i].skew_after > max_skew, vs[i].skew_after, len(vs[i].moves),
                                                     vs[i].moved_cpu_m, i))
    best = vs[report.best]
    assignment = dict(plan.assignment)
    for svc, _, dst in best.moves:
        assignment[svc] = dst
    relaxed = {svc: keys for svc, keys in plan.relaxed.items() if svc not in {m[0] for m in best.moves}}
    relaxed.update(best.relaxed)  # a moved service carries the keys its move gave up, and no others
    report.plan = dataclasses.replace(plan, assignment=assignment, relaxed=relaxed)
    return report


@dataclass
class GrowCandidate:
    """One candidate of a scale-out sweep (SPEC.md 2.12): a server template and what adding servers of it does
    for the plan's unplaced services."""
    name: str
    cpu_m: int
    mem_mib: int
    labels: list[str]                      # the template's labels the stage knows; others are dropped
    max_new: int = 0                       # the most new servers the candidate could open
    pending: int = 0                       # the eight words of the summary row
    placed: int = 0
    opened: int = 0
    unplaceable: int = 0
    capped: int = 0
    left_cpu_m: int = 0
    left_mem_mib: int = 0
    first_unplaced: str | None = None      # the first service in visiting order that gets no server
    # the services of each new server in visiting order (cpu desc, mem desc, stage order); None where the
    # candidate was not detailed
    servers: list[list[str]] | None = None
    # under the policy (SPEC.md 2.18, grow_stage(under_policy=True)); unset otherwise
    on_live: int | None = None             # pending services that land on an EXISTING server
    relaxed: dict[str, list[str]] = field(default_factory=dict)  # placed service -> label keys given up (Plan.relaxed)
    stuck_skew: int | None = None          # pending services some server fits and none takes within the skew
    stuck_quota: int | None = None         # pending services the quota refuses
    skew_before: int | None = None         # max - min of the services per eligible domain, the new servers' included
    skew_after: int | None = None          # the same after the placements
    domain: str | None = None              # the template's "key=value" under the constraint's topology key
    moved_in: list[tuple[str, str]] = field(default_factory=list)  # (service, existing server) in visiting order
    no_topology_key: bool = False          # under a constraint a template without the key is no candidate


@dataclass
class GrowReport:
    """``grow_stage``'s answer: one GrowCandidate per template of the catalogue, every one computed
    independently for the same pending services."""
    stage: str
    max_new: int = 0
    pending: list[str] = field(default_factory=list)  # the plan's NOFIT services, stage order
    candidates: list[GrowCandidate] = field(default_factory=list)
    # the policy the answer was held to (SPEC.md 2.18); unset without under_policy, where ``pending`` holds the
    # plan's NOFIT and SKEW services
    under_policy: bool = False
    strategy: str | None = None
    preferred: list[str] = field(default_factory=list)
    spread_topology_key: str | None = None
    spread_max_skew: int | None = None
    fallback_relax_order: list[str] = field(default_factory=list)
    fallback_max_hops: int | None = None
    quota: tuple | None = None
    quota_used: tuple | None = None


def _grow_stage_policy(flow: Flow, stage_name: str, plan: Plan, catalogue: list[Server], max_new: int, p: Planner,
                       policy: PlacementPolicy | None) -> GrowReport:
    """``grow_stage(under_policy=True)``: SPEC.md 2.18, one ``Planner.grow_sweep_policy`` call."""
    from ._lib import (FP_SPREAD_MAX_DOMAINS, GROW_CAPPED, GROW_FIRST_UNPLACED, GROW_LEFT_CPU, GROW_LEFT_MEM, GROW_ON_LIVE,
                       GROW_OPENED, GROW_PENDING, GROW_PLACED, GROW_SKEW_AFTER, GROW_SKEW_BEFORE, GROW_STUCK_QUOTA,
                       GROW_STUCK_SKEW, GROW_UNPLACEABLE, REASON_NOFIT, REASON_OK, REASON_SKEW)
    pol = policy if policy is not None else _plan_policy(plan)
    names, nodes, cont, live, _, count, strategy, pmask = live_tables(flow, stage_name, plan, pol)
    ld = _stage_labels(names, flow, nodes, pol.preferred)
    code = {"NOFIT": REASON_NOFIT, "SKEW": REASON_SKEW}
    reason = [code.get(plan.rejected.get(n), REASON_OK) for n in names]
    report = GrowReport(stage_name, int(max_new), [n for n, r in zip(names, reason) if r != REASON_OK], [], True,
                        strategy, pol.preferred)
    if pol.fallback:
        report.fallback_relax_order, report.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    used = tuple(plan.quota_used) if plan.quota_used is not None else (0, 0, 0)
    if pol.quota is not None:
        report.quota, report.quota_used = pol.quota, used
    domain, max_skew, t_value = None, 0, [None] * len(catalogue)
    cand = list(range(len(catalogue)))  # the templates that are candidates, catalogue order
    t_domain = None
    if pol.spread is not None:
        key, max_skew = pol.spread
        report.spread_topology_key, report.spread_max_skew = key, max_skew
        domain, has_key = replan_domains(nodes, key)
        live = (*live[:4], [s if k else 0 for s, k in zip(live[4], has_key)])
        prefix = key + "="
        ids = {}
        for nd, d, k in zip(nodes, domain, has_key):
            if k:
                ids.setdefault(next(lab for lab in nd.labels if lab.startswith(prefix)), d)
        nxt = max(domain, default=-1) + 1  # past the spare id of the servers without the key
        t_value = [next((lab for lab in t.labels if lab.startswith(prefix)), None) for t in catalogue]
        cand = [k for k, v in enumerate(t_value) if v is not None]
        t_domain = []
        for k in cand:
            if t_value[k] not in ids:
                ids[t_value[k]] = nxt
                nxt += 1
            t_domain.append(ids[t_value[k]])
        if nxt > FP_SPREAD_MAX_DOMAINS:
            raise ValueError(f"spread constraint: the stage and the catalogue have {nxt} distinct domains under "
                             f"'{key}' (at most {FP_SPREAD_MAX_DOMAINS})")
    known = [[lab for lab in t.labels if lab in ld.bits] for t in catalogue]
    for t, labs, value in zip(catalogue, known, t_value):
        c = GrowCandidate(t.slug, t.cpu_m, t.mem_mib, labs, int(max_new), len(report.pending))
        c.domain, c.no_topology_key = value, pol.spread is not None and value is None
        report.candidates.append(c)
    if not cand:
        return report
    tpl = ([catalogue[k].cpu_m for k in cand], [catalogue[k].mem_mib for k in cand], [ld.mask(known[k]) for k in cand])
    relax = [ld.key_mask(k) for k in pol.fallback]
    summary, rows, assign, hops, _ = p.grow_sweep_policy(
        cont, reason, live, tpl, max_new, (1 << REASON_NOFIT) | (1 << REASON_SKEW), None,
        strategy if strategy is not None else 0, pmask, count, domain=domain, t_domain=t_domain, max_skew=max_skew,
        relax_mask=relax, quota=pol.quota, quota_used=used if pol.quota is not None else None, want_assign=True)
    visit = sorted((v for v, r in enumerate(reason) if r != REASON_OK), key=lambda v: (-cont[0][v], -cont[1][v], v))
    N = len(nodes)
    for j, k in enumerate(cand):
        c, row, prow = report.candidates[k], [int(x) for x in summary[j]], [int(x) for x in rows[j]]
        first = row[GROW_FIRST_UNPLACED]
        c.pending, c.placed, c.opened, c.unplaceable, c.capped = (row[GROW_PENDING], row[GROW_PLACED], row[GROW_OPENED],
                                                                  row[GROW_UNPLACEABLE], row[GROW_CAPPED])
        c.left_cpu_m, c.left_mem_mib = row[GROW_LEFT_CPU], row[GROW_LEFT_MEM]
        c.first_unplaced = names[first] if first != NONE else None
        c.on_live, c.stuck_skew, c.stuck_quota = prow[GROW_ON_LIVE], prow[GROW_STUCK_SKEW], prow[GROW_STUCK_QUOTA]
        if pol.spread is not None:
            c.skew_before, c.skew_after = prow[GROW_SKEW_BEFORE], prow[GROW_SKEW_AFTER]
        c.servers = [[] for _ in range(c.opened)]
        for v in visit:
            n = int(assign[j][v])
            if n == NONE:
                continue
            if n < N:
                c.moved_in.append((names[v], nodes[n].slug))
            else:
                c.servers[n - N].append(names[v])  # the new servers used are [N, N + opened)
            if int(hops[j][v]):
                required = {lab.split("=", 1)[0] for lab in flow.services.get(names[v], Service()).labels}
                c.relaxed[names[v]] = [key for key in pol.fallback[:int(hops[j][v])] if key in required]
    return report


def grow_stage(flow: Flow, stage_name: str, plan: Plan, catalogue: list[Server], max_new: int = 64,
               planner: Planner | None = None, policy: PlacementPolicy | None = None,
               under_policy: bool = False) -> GrowReport:
    """"What do I have to add?" for a stage planned as ``plan`` says (SPEC.md 2.12): the pending services are
    the plan's NOFIT rejections, with their full required labels, and every ``Server`` of ``catalogue``
    (``registry.plan_template``) is a template of which up to ``max_new`` new servers may be opened, first
    fit.  Template labels go through the stage's label dictionary; a label nothing in the stage uses is
    dropped.  One ``Planner.grow_sweep`` covers the catalogue; a second one, with the per-server lists,
    covers the templates that place every pending service or, when none does, the one that places the most
    (the first of them in catalogue order).  The policy's strategy, preferred labels, spread constraint,
    fallback chain and quota are not applied by default.

    ``under_policy=True`` applies them (SPEC.md 2.18, one ``Planner.grow_sweep_policy`` call): those of
    ``policy`` or, without one, of the policy the plan was made under, with the quota's usage the plan left.
    The pending services are then the plan's NOFIT **and SKEW** rejections, and each template's servers are
    added behind the live tables of ``live_tables``, so a pending service may land on an existing server
    (``GrowCandidate.moved_in``).  Under a spread constraint a template stands in the domain its
    ``topology_key=value`` label names, in the stage's numbering; a value the stage does not have is a new
    domain (a 65th is a ValueError), and a template without the key is no candidate: it is reported with
    nothing placed and ``no_topology_key``.  Every candidate is detailed."""
    if under_policy:
        return _grow_stage_policy(flow, stage_name, plan, catalogue, max_new, planner or default_planner(), policy)
    from ._lib import (GROW_CAPPED, GROW_FIRST_UNPLACED, GROW_LEFT_CPU, GROW_LEFT_MEM, GROW_OPENED, GROW_PENDING,
                       GROW_PLACED, GROW_UNPLACEABLE, REASON_NOFIT, REASON_OK)
    p = planner or default_planner()
    stage = flow.stages[stage_name]
    names = list(dict.fromkeys(stage.services))
    nodes = _server_nodes(flow, stage.servers)
    cont, _ = _stage_tables(names, flow, nodes, plan.preferred)
    ld = _stage_labels(names, flow, nodes, plan.preferred)
    reason = [REASON_NOFIT if plan.rejected.get(n) == "NOFIT" else REASON_OK for n in names]
    report = GrowReport(stage_name, int(max_new), [n for n, r in zip(names, reason) if r == REASON_NOFIT])
    if not catalogue:
        return report
    known = [[lab for lab in t.labels if lab in ld.bits] for t in catalogue]
    tpl = ([t.cpu_m for t in catalogue], [t.mem_mib for t in catalogue], [ld.mask(k) for k in known])
    summary, _ = p.grow_sweep(cont, reason, tpl, max_new)
    for t, labs, row in zip(catalogue, known, summary):
        row = [int(x) for x in row]
        first = row[GROW_FIRST_UNPLACED]
        report.candidates.append(GrowCandidate(
            t.slug, t.cpu_m, t.mem_mib, labs, int(max_new), row[GROW_PENDING], row[GROW_PLACED], row[GROW_OPENED],
            row[GROW_UNPLACEABLE], row[GROW_CAPPED], row[GROW_LEFT_CPU], row[GROW_LEFT_MEM],
            names[first] if first != NONE else None))
    if not report.pending:
        return report
    detail = [k for k, c in enumerate(report.candidates) if c.placed == c.pending]
    if not detail:
        detail = [max(range(len(catalogue)), key=lambda k: (report.candidates[k].placed, -k))]
    _, assign = p.grow_sweep(cont, reason, tuple([x[k] for k in detail] for x in tpl), max_new, want_assign=True)
    visit = sorted((v for v, r in enumerate(reason) if r == REASON_NOFIT), key=lambda v: (-cont[0][v], -cont[1][v], v))
    for k, row in zip(detail, assign):
        c = report.candidates[k]
        c.servers = [[] for _ in range(c.opened)]
        for v in visit:
            if int(row[v]) != NONE:
                c.servers[int(row[v])].append(names[v])
    return report


@dataclass
class Replan:
    """``replan_stage``'s answer (SPEC.md 2.13, 2.14): the stage's next plan and what it changes for the services
    that ran under the previous one.  Services are listed in stage order."""
    plan: Plan                                  # goes straight into drain_stage, grow_stage or the next replan_stage
    kept: list[str] = field(default_factory=list)                    # stayed on their server
    new: list[str] = field(default_factory=list)                     # did not run before, placed now
    moved: list[tuple[str, str, str]] = field(default_factory=list)  # (service, from, to)
    # (service, from, "NOFIT" | "CYCLE"; under the policy, SPEC.md 2.14, "SKEW" | "QUOTA" as well)
    lost: list[tuple[str, str, str]] = field(default_factory=list)
    moved_cpu_m: int = 0                        # what the moved services ask for in sum: the migration volume
    moved_mem_mib: int = 0
    # SPEC.md 2.14: kept seats are never evicted, so they alone may leave the stage outside a guarantee.  The
    # final max - min of the eligible domains' counts when it exceeds max_skew (else None), and the quota
    # dimensions ("cpu", "memory", "services") whose usage ends above their cap
    skew_excess: int | None = None
    quota_over: list[str] = field(default_factory=list)


def _hard_guarantees(policy: PlacementPolicy | None, plan: Plan) -> list[str]:
    """The hard guarantees of ``policy`` -- or, without one, of the policy ``plan`` was made under -- that a
    re-plan would not apply (SPEC.md 2.13)."""
    if policy is not None:
        found = (policy.spread is not None, bool(policy.fallback), policy.quota is not None)
    else:
        found = (plan.spread_topology_key is not None and bool(plan.spread_max_skew), bool(plan.fallback_relax_order)
                 and plan.fallback_max_hops != 0, plan.quota is not None)
    return [name for name, there in zip(("spread constraint", "fallback chain", "resource quota"), found) if there]


def replan_domains(nodes: list[Server], topology_key: str) -> tuple[list[int], list[bool]]:
    """``spread_domains`` for a re-plan (SPEC.md 2.14).  A server without the key is no candidate, but pass 1
    ignores ``schedulable``: what runs on it stays and is counted in its domain, and ``spread_domains``' id 0
    would count it into the first value's domain.  Keyless servers get one spare id, the next unused one: it has
    no schedulable server, so it is never eligible and its count is never read.  64 values and a keyless server
    leave no spare id: a ValueError."""
    from ._lib import FP_SPREAD_MAX_DOMAINS
    domain, has_key = spread_domains(nodes, topology_key)
    if all(has_key):
        return domain, has_key
    spare = max((d for d, k in zip(domain, has_key) if k), default=-1) + 1
    if spare >= FP_SPREAD_MAX_DOMAINS:
        raise ValueError(f"spread constraint: topology key '{topology_key}' has {spare} distinct values in this stage "
                         f"and a server without the key: a re-plan needs a spare domain id for it (at most "
                         f"{FP_SPREAD_MAX_DOMAINS} in all)")
    return [d if k else spare for d, k in zip(domain, has_key)], has_key


def _plan_policy(plan: Plan) -> PlacementPolicy:
    """The policy ``plan`` was made under, rebuilt from its fields."""
    caps = plan.quota if plan.quota is not None else (None, None, None)
    return PlacementPolicy(plan.strategy, dict(lab.split("=", 1) for lab in plan.preferred), plan.spread_topology_key,
                           plan.spread_max_skew, tuple(plan.fallback_relax_order), plan.fallback_max_hops, *caps)


def replan_stage(flow: Flow, stage_name: str, plan: Plan, planner: Planner | None = None,
                 policy: PlacementPolicy | None = None, under_policy: bool = False, quota_used=None) -> Replan:
    """The next plan of a stage that runs as ``plan`` says (SPEC.md 2.13; with ``under_policy``, 2.14): `fleet up`
    on a running stage.  The tables are built as ``plan_stage`` builds them, from the flow as it is now (new
    requests, new servers); a service keeps the server ``plan.assignment`` names while it still fits there -- on a
    cordoned server too -- and one ``Planner.replan`` call (``Planner.replan_policy`` with ``under_policy``) places
    the others under the strategy and preferred labels of ``policy`` or, without one, of the policy the plan was
    made under.  Levels and orders are computed as in ``plan_stage``.

    A service whose old server is no longer in the stage, or is flagged ``draining``, has no seat to keep: it
    goes to the planner as one that does not run, and is reported here as moved (from its old slug) or lost.

    By default the spread constraint, the fallback chain and the quota are not applied by a re-plan, and a new
    plan must not silently drop a hard guarantee: a ``policy`` that carries one, or without a policy a ``plan``
    made under one, is a ValueError that names it.

    ``under_policy=True`` applies them (SPEC.md 2.14, one ``Planner.replan_policy`` call): the guarantees of
    ``policy`` or, without one, those rebuilt from the plan's ``spread_*``, ``fallback_*`` and ``quota`` fields.
    ``quota_used`` is what the tenant holds outside this stage, as in ``plan_stage`` (default zeros);
    ``plan.quota_used`` is the usage after that plan and is not the base.  Seats are kept without a skew or
    quota test and are counted and charged; only new and moved services are held to the guarantees, and may be
    rejected "SKEW" or "QUOTA".  The returned plan carries ``relaxed``, ``quota``, ``quota_used`` and
    ``quota_why`` as ``plan_stage`` fills them, and ``Replan.skew_excess`` / ``Replan.quota_over`` say where the
    seats alone leave the stage outside a guarantee.  Servers without the topology key take no new service, but
    keep what runs on them (``replan_domains``)."""
    from ._lib import (CHANGE_KEPT, CHANGE_LOST, CHANGE_MOVED, CHANGE_NEW, QUOTA_NAMES, REPLAN_MOVED_CPU,
                       REPLAN_MOVED_MEM)
    pol = None
    if under_policy:
        pol = policy if policy is not None else _plan_policy(plan)
    hard = [] if under_policy else _hard_guarantees(policy, plan)
    if hard:
        raise ValueError(f"replan of stage '{stage_name}': the {' and the '.join(hard)} of the "
                         f"{'policy' if policy is not None else 'plan'} would not be applied (SPEC.md 2.13); "
                         "plan the stage afresh with plan_stage, or pass a policy without it")
    p = planner or default_planner()
    stage = flow.stages[stage_name]
    services = list(stage.services)
    nodes = _server_nodes(flow, stage.servers)
    strategy = policy.strategy if policy is not None else plan.strategy
    preferred = policy.preferred if policy is not None else list(plan.preferred)
    if not services:
        return Replan(Plan(stage_name, [], {}, [], {}, {}, strategy=strategy, preferred=preferred))
    names, pos2v, row_ptr, col, has_deps = stage_graph(services, flow)
    if len(names) == len(services):
        perm, level_v, order_v, _, _ = p.plan_stage(row_ptr, col, has_deps)
        order = [services[i] for i in perm.tolist()]
        levels = level_v.tolist()
        level_order = [services[i] for i in order_v.tolist()]
    else:
        order = order_by_dependencies(services, flow, p)
        levels, level_order = levelize_stage(services, flow, p)
    lvl_v = {names[v]: levels[i] for i, v in enumerate(pos2v)}
    new_plan = Plan(stage_name, order, dict(zip(services, levels)), level_order, {}, {}, strategy=strategy,
                    preferred=preferred)
    out = Replan(new_plan)
    slugs = [nd.slug for nd in nodes]
    index = {s: n for n, s in enumerate(slugs)}
    prev, gone = [NONE] * len(names), {}
    for v, name in enumerate(names):
        slug = plan.assignment.get(name)
        if slug is None:
            continue
        if slug not in index or nodes[index[slug]].draining:
            gone[name] = slug
        else:
            prev[v] = index[slug]
    if not nodes:  # nothing to place on, as in plan_stage: whatever ran is lost
        out.lost = [(n, gone[n], "CYCLE" if lvl_v[n] == NONE else "NOFIT") for n in names if n in gone]
        return out
    cont, ntab = _stage_tables(names, flow, nodes, preferred)
    pmask = _stage_labels(names, flow, nodes, preferred).mask(preferred)
    if pol is None:
        assign, reason, change, summary, _, _ = p.replan(cont, ntab, prev, strategy if strategy is not None else 0, pmask,
                                                         level=[lvl_v[n] for n in names])
    else:
        domain, max_skew = None, 0
        if pol.spread is not None:
            domain, has_key = replan_domains(nodes, pol.spread[0])
            max_skew = pol.spread[1]
            ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
            new_plan.spread_topology_key, new_plan.spread_max_skew = pol.spread
        ld = _stage_labels(names, flow, nodes, preferred)
        relax = [ld.key_mask(k) for k in pol.fallback]
        base = (0, 0, 0) if quota_used is None else tuple(int(x) for x in quota_used)
        assign, reason, hops, change, summary, _, counts, qwhy, qused = p.replan_policy(
            cont, ntab, prev, strategy if strategy is not None else 0, pol.quota, base, relax, preferred=pmask,
            level=[lvl_v[n] for n in names], node_count=[0] * len(nodes), domain=domain, max_skew=max_skew)
        if pol.fallback:
            new_plan.fallback_relax_order, new_plan.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
            for v, n in enumerate(names):
                if int(assign[v]) != NONE and int(hops[v]):
                    required = {lab.split("=", 1)[0] for lab in flow.services.get(n, Service()).labels}
                    new_plan.relaxed[n] = [k for k in pol.fallback[:int(hops[v])] if k in required]
        if pol.quota is not None:
            new_plan.quota, new_plan.quota_used = pol.quota, tuple(int(x) for x in qused)
            new_plan.quota_why = {n: [d for k, d in enumerate(QUOTA_NAMES) if int(qwhy[v]) >> k & 1]
                                  for v, n in enumerate(names) if int(reason[v]) == 4}
            out.quota_over = [d for d, cap, u in zip(QUOTA_NAMES, pol.quota, new_plan.quota_used)
                              if cap is not None and u > cap]
        if pol.spread is not None:
            per, eligible = {}, set()
            for n, d in enumerate(domain):
                per[d] = per.get(d, 0) + int(counts[n])
                if ntab[4][n]:
                    eligible.add(d)
            if eligible:
                skew = max(per[d] for d in eligible) - min(per[d] for d in eligible)
                out.skew_excess = skew if skew > max_skew else None
    out.moved_cpu_m, out.moved_mem_mib = int(summary[REPLAN_MOVED_CPU]), int(summary[REPLAN_MOVED_MEM])
    for v, name in enumerate(names):
        why = {2: "CYCLE", 3: "SKEW", 4: "QUOTA"}.get(int(reason[v]), "NOFIT")
        if int(assign[v]) != NONE:
            new_plan.assignment[name] = slugs[int(assign[v])]
        else:
            new_plan.rejected[name] = why
        chg = int(change[v])
        if chg == CHANGE_KEPT:
            out.kept.append(name)
        elif chg == CHANGE_MOVED:
            out.moved.append((name, slugs[prev[v]], slugs[int(assign[v])]))
        elif chg == CHANGE_LOST:
            out.lost.append((name, slugs[prev[v]], why))
        elif name in gone:  # NEW or ABSENT at the ABI: it ran, on a server it cannot stay on
            if chg == CHANGE_NEW:
                out.moved.append((name, gone[name], slugs[int(assign[v])]))
                out.moved_cpu_m = (out.moved_cpu_m + cont[0][v]) & U32_MAX
                out.moved_mem_mib = (out.moved_mem_mib + cont[1][v]) & U32_MAX
            else:
                out.lost.append((name, gone[name], why))
        elif chg == CHANGE_NEW:
            out.new.append(name)
    return out


def resolve_target_server(flow: Flow, stage_name: str, planner: Planner | None = None) -> str | None:
    """handlers/deploy.rs:390-394: ``flow.stages.get(stage).and_then(|s| s.servers.first().cloned())``.

    Computed as FFD over the stage's servers with unconstrained capacity: every
    service lands on node 0.  An empty or missing stage/server list gives None
    (the caller records "local", :396-398)."""
    stage = flow.stages.get(stage_name)
    if stage is None or not stage.servers:
        return None
    p = planner or default_planner()
    n = max(1, len(stage.services))
    nodes = ([U32_MAX] * len(stage.servers), [U32_MAX] * len(stage.servers), [0] * len(stage.servers),
             [0] * len(stage.servers), [1] * len(stage.servers))
    assign, _, _ = p.place(([0] * n, [0] * n, [0] * n, [0] * n), nodes)
    return stage.servers[int(assign[0])]
