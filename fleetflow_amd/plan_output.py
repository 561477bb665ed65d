"""Plan output: JSON plan and the dry-run presenter.

``plan_to_json`` is the machine form carried to the control plane next to
``DeployRequest`` (crates/fleetflow-container/src/engine.rs:16-25):
``{stage, order, levels, level_order, assign, rejected}``, and for a plan made under a placement
policy ``placement`` (``strategy``, ``preferred``, ``spread``, ``fallback``) and, under a fallback chain
(SPEC.md 2.8), ``relaxed``: the label keys each relaxed service gave up.  A plan made with
``plan_stage(..., explain=True)`` carries ``why``: the rejection diagnosis (SPEC.md 2.9) of each service
rejected NOFIT or SKEW; the key is absent when there is none.  A plan made under a resource quota
(SPEC.md 2.10) carries ``quota`` (``caps`` and the usage after the plan, ``used``, per dimension; a null
cap is none) and ``quota_why``: the dimensions that refused each service rejected QUOTA.  Both keys are
absent without a quota.

``format_drain_report`` prints a drain sweep (SPEC.md 2.11, ``flow.drain_stage``), one block per candidate,
and ``drain_report_to_json`` / ``drain_report_from_json`` carry it as
``{stage, by, placement: {strategy, preferred}, candidates: [{name, servers, moves, stranded, ...}]}``; a sweep
under the policy (SPEC.md 2.15) adds ``placement.spread`` / ``placement.fallback`` and per candidate ``relaxed``,
``stranded_reason``, ``skew_before`` and ``skew_after``, each only when set.

``format_grow_report`` prints a scale-out sweep (SPEC.md 2.12, ``flow.grow_stage``), one line per template with
the services of each new server indented under it where the candidate was detailed, and ``grow_report_to_json``
/ ``grow_report_from_json`` carry it as ``{stage, max_new, pending, candidates: [{name, cpu_m, ...}]}``.

``format_shrink_report`` prints a scale-in sweep (SPEC.md 2.16, ``flow.shrink_stage``), one block per release order,
and ``shrink_report_to_json`` / ``shrink_report_from_json`` carry it as ``{stage, placement: {strategy, preferred},
keep, best, plan, variants: [{name, order, released, moves, stayed, ...}]}`` with ``plan`` in ``plan_to_json``'s form;
a sweep under the policy (SPEC.md 2.17) adds ``placement.spread`` / ``placement.fallback`` and per variant ``relaxed``,
``stayed_reason``, ``skew_before`` and ``skew_after``, each only when set.

``format_replan_report`` prints a re-plan (SPEC.md 2.13, ``flow.replan_stage``): one line of counts, then the
moves, the new and the lost services, and ``replan_report_to_json`` / ``replan_report_from_json`` carry it as
``{plan, kept, new, moved, lost, moved_cpu_m, moved_mem_mib}`` with ``plan`` in ``plan_to_json``'s form.

``format_up_dry_run`` / ``format_deploy_dry_run`` reproduce the reference's
``fleet up --dry-run`` (crates/fleetflow/src/commands/up.rs:57-136) and
``fleet deploy --dry-run`` (crates/fleetflow/src/commands/deploy.rs:14-100)
line for line, without ANSI colour. When a ``Plan`` is given, each service
block gains its start level, its candidate servers (stage 2: the feasible-server count
and the first feasible server on the pristine table) and its planned server. Without one the
text is the reference's. The environment line lists variables in definition
order (the reference iterates a HashMap, so its order is arbitrary; compare it
as a set).
"""
from __future__ import annotations

import json

from dataclasses import asdict

from ._lib import QUOTA_NAMES
from .flow import (U32_MAX, WHY_NAMES, DrainCandidate, DrainReport, Flow, GrowCandidate, GrowReport, Plan,
                   RebalanceReport, RebalanceVariant, Replan, ShrinkReport, ShrinkVariant, Why)
from .parser import FlowError


def plan_to_json(plan: Plan, indent: int | None = None) -> str:
    """Serialise a plan; a cycle member's level is null (it was U32_MAX)."""
    d = {
        "stage": plan.stage,
        "order": plan.order,
        "levels": {k: (None if v == U32_MAX else v) for k, v in plan.levels.items()},
        "level_order": plan.level_order,
        "assign": plan.assignment,
        "rejected": plan.rejected,
        "candidates": {k: {"count": c, "first": f} for k, (c, f) in plan.candidates.items()},
    }
    spread = plan.spread_topology_key is not None
    fallback = bool(plan.fallback_relax_order)
    if plan.strategy is not None or plan.preferred or spread or fallback:  # made under a placement policy (SPEC.md 2.6-2.8)
        d["placement"] = {"strategy": plan.strategy, "preferred": plan.preferred}
        if spread:
            d["placement"]["spread"] = {"topology_key": plan.spread_topology_key, "max_skew": plan.spread_max_skew}
        if fallback:
            d["placement"]["fallback"] = {"relax_order": plan.fallback_relax_order, "max_hops": plan.fallback_max_hops}
            d["relaxed"] = plan.relaxed
    if plan.why:  # rejection diagnosis (SPEC.md 2.9)
        d["why"] = {k: asdict(w) for k, w in plan.why.items()}
    if plan.quota is not None:  # resource quota (SPEC.md 2.10)
        d["quota"] = {"caps": dict(zip(QUOTA_NAMES, plan.quota)),
                      "used": dict(zip(QUOTA_NAMES, plan.quota_used)) if plan.quota_used is not None else None}
        d["quota_why"] = plan.quota_why
    return json.dumps(d, ensure_ascii=False, indent=indent)


def plan_from_json(text: str) -> Plan:
    d = json.loads(text)
    pol = d.get("placement") or {}
    q = d.get("quota")
    plan = Plan(d["stage"], d["order"], {k: (U32_MAX if v is None else v) for k, v in d["levels"].items()},
                d["level_order"], d["assign"], d["rejected"],
                {k: (v["count"], v["first"]) for k, v in d.get("candidates", {}).items()},
                pol.get("strategy"), list(pol.get("preferred") or []),
                (pol.get("spread") or {}).get("topology_key"), (pol.get("spread") or {}).get("max_skew"),
                list((pol.get("fallback") or {}).get("relax_order") or []), (pol.get("fallback") or {}).get("max_hops"),
                {k: list(v) for k, v in (d.get("relaxed") or {}).items()},
                {k: Why(dict(w["fail"]), dict(w["only"]), w["feasible"], list(w["universal"]), list(w["missing_labels"]),
                        w["nearest"], w.get("servers", 0)) for k, w in (d.get("why") or {}).items()})
    if q is not None:
        plan.quota = tuple(q["caps"].get(n) for n in QUOTA_NAMES)
        plan.quota_used = tuple(q["used"][n] for n in QUOTA_NAMES) if q.get("used") is not None else None
        plan.quota_why = {k: list(v) for k, v in (d.get("quota_why") or {}).items()}
    return plan


def format_drain_report(report: DrainReport) -> str:
    """One line per candidate, ``drain <name>: <m> services move to <t> servers, <s> stranded``, with the
    moves (``service: from -> to``) and the stranded services indented under it, in visiting order.  What a
    sweep under the policy adds (SPEC.md 2.15) is printed only where it is set: ``(relaxed: class)`` behind a
    move, ``stranded (SKEW)``, and a ``spread:`` line for a candidate whose remaining servers are outside the
    constraint before anything moves."""
    lines = []
    for c in report.candidates:
        lines.append(f"drain {c.name}: {len(c.moves)} services move to {c.targets} servers, {len(c.stranded)} stranded")
        lines += [f"  {svc}: {src} -> {dst}" + (f" (relaxed: {', '.join(c.relaxed[svc])})" if c.relaxed.get(svc) else "")
                  for svc, src, dst in c.moves]
        lines += [f"  {svc}: stranded" + (f" ({c.stranded_reason[svc]})" if svc in c.stranded_reason else "")
                  for svc in c.stranded]
        if (c.skew_before is not None and report.spread_max_skew is not None
                and c.skew_before > report.spread_max_skew):
            lines.append(f"  spread: skew {c.skew_before} over {report.spread_topology_key} exceeds max_skew "
                         f"{report.spread_max_skew} (services that stay are not evicted)")
    return "\n".join(lines)


_DRAIN_POLICY_FIELDS = ("relaxed", "stranded_reason", "skew_before", "skew_after")


def drain_report_to_json(report: DrainReport, indent: int | None = None) -> str:
    cands = []
    for c in report.candidates:
        row = asdict(c)
        for key in _DRAIN_POLICY_FIELDS:  # SPEC.md 2.15: only when set
            if not row[key] and row[key] != 0:
                del row[key]
        cands.append(row)
    d = {"stage": report.stage, "by": report.by,
         "placement": {"strategy": report.strategy, "preferred": report.preferred},
         "candidates": cands}
    if report.spread_topology_key is not None:
        d["placement"]["spread"] = {"topology_key": report.spread_topology_key, "max_skew": report.spread_max_skew}
    if report.fallback_relax_order:
        d["placement"]["fallback"] = {"relax_order": report.fallback_relax_order, "max_hops": report.fallback_max_hops}
    return json.dumps(d, ensure_ascii=False, indent=indent)


def drain_report_from_json(text: str) -> DrainReport:
    d = json.loads(text)
    pol = d.get("placement") or {}
    cands = [DrainCandidate(c["name"], list(c["servers"]), [tuple(m) for m in c["moves"]], list(c["stranded"]),
                            c.get("evicted", 0), c.get("stranded_cpu_m", 0), c.get("stranded_mem_mib", 0),
                            c.get("targets", 0), {k: list(v) for k, v in (c.get("relaxed") or {}).items()},
                            dict(c.get("stranded_reason") or {}), c.get("skew_before"), c.get("skew_after"))
             for c in d.get("candidates") or []]
    return DrainReport(d["stage"], d.get("by"), pol.get("strategy"), list(pol.get("preferred") or []), cands,
                       (pol.get("spread") or {}).get("topology_key"), (pol.get("spread") or {}).get("max_skew"),
                       list((pol.get("fallback") or {}).get("relax_order") or []),
                       (pol.get("fallback") or {}).get("max_hops"))


def format_shrink_report(report: ShrinkReport) -> str:
    """One line per release order, ``shrink <name>: <r> of <t> servers released, <m> services move (<cpu>m cpu,
    <mem> MiB), <f> attempts undone``, marked ``(best)`` where it is, with the released servers
    (``released: a, b``), the moves (``service: from -> to``) and the servers that stayed (``server: stays
    (blocked by service)``) indented under it.  What a sweep under the policy adds (SPEC.md 2.17) is printed only
    where it is set: ``(relaxed: class)`` behind a move, ``stays (blocked by service, SKEW)``, ``stays (bound
    rule: ...)`` for a server whose services all found a place and whose release the spread constraint refuses,
    and a ``spread:`` line with the skew before and after."""
    lines = []
    for i, v in enumerate(report.variants):
        lines.append(f"shrink {v.name}: {len(v.released)} of {v.tried} servers released, {len(v.moves)} services move "
                     f"({v.moved_cpu_m}m cpu, {v.moved_mem_mib} MiB), {v.failed} attempts undone"
                     + (" (best)" if i == report.best else ""))
        if v.released:
            lines.append(f"  released: {', '.join(v.released)}")
        lines += [f"  {svc}: {src} -> {dst}" + (f" (relaxed: {', '.join(v.relaxed[svc])})" if v.relaxed.get(svc) else "")
                  for svc, src, dst in v.moves]
        for srv, svc in v.stayed:
            why = v.stayed_reason.get(srv)
            if svc is None:
                lines.append(f"  {srv}: stays (bound rule: its release would leave the skew over "
                             f"{report.spread_topology_key} above max_skew {report.spread_max_skew} and above what it is)")
            else:
                lines.append(f"  {srv}: stays (blocked by {svc}" + (f", {why}" if why else "") + ")")
        if v.skew_before is not None:
            lines.append(f"  spread: skew over {report.spread_topology_key} {v.skew_before} -> {v.skew_after} "
                         f"(max_skew {report.spread_max_skew})")
    return "\n".join(lines)


_SHRINK_POLICY_FIELDS = ("relaxed", "stayed_reason", "skew_before", "skew_after")


def shrink_report_to_json(report: ShrinkReport, indent: int | None = None) -> str:
    variants = []
    for v in report.variants:
        row = asdict(v)
        for key in _SHRINK_POLICY_FIELDS:  # SPEC.md 2.17: only when set
            if not row[key] and row[key] != 0:
                del row[key]
        variants.append(row)
    d = {"stage": report.stage, "placement": {"strategy": report.strategy, "preferred": report.preferred},
         "keep": report.keep, "best": report.best,
         "plan": None if report.plan is None else json.loads(plan_to_json(report.plan)),
         "variants": variants}
    if report.spread_topology_key is not None:
        d["placement"]["spread"] = {"topology_key": report.spread_topology_key, "max_skew": report.spread_max_skew}
    if report.fallback_relax_order:
        d["placement"]["fallback"] = {"relax_order": report.fallback_relax_order, "max_hops": report.fallback_max_hops}
    return json.dumps(d, ensure_ascii=False, indent=indent)


def shrink_report_from_json(text: str) -> ShrinkReport:
    d = json.loads(text)
    pol = d.get("placement") or {}
    variants = [ShrinkVariant(v["name"], list(v["order"]), list(v["released"]), [tuple(m) for m in v["moves"]],
                              [tuple(x) for x in v["stayed"]], v.get("tried", 0), v.get("failed", 0), v.get("n_moves", 0),
                              v.get("moved_cpu_m", 0), v.get("moved_mem_mib", 0),
                              {k: list(x) for k, x in (v.get("relaxed") or {}).items()},
                              dict(v.get("stayed_reason") or {}), v.get("skew_before"), v.get("skew_after"))
                for v in d.get("variants") or []]
    plan = d.get("plan")
    return ShrinkReport(d["stage"], pol.get("strategy"), list(pol.get("preferred") or []), list(d.get("keep") or []),
                        variants, d.get("best"),
                        None if plan is None else plan_from_json(json.dumps(plan, ensure_ascii=False)),
                        (pol.get("spread") or {}).get("topology_key"), (pol.get("spread") or {}).get("max_skew"),
                        list((pol.get("fallback") or {}).get("relax_order") or []),
                        (pol.get("fallback") or {}).get("max_hops"))


def format_rebalance_report(report: RebalanceReport) -> str:
    """One line per victim order, ``rebalance <name>: <m> services move (<cpu>m cpu, <mem> MiB), skew over <key>
    <before> -> <after> (max_skew <k>), <s> attempts refused``, marked ``(best)`` where it is and with ``budget
    <b>`` where the variant had one, with the moves (``service: from -> to``, ``(relaxed: class)`` behind a relaxed
    one) and the services that stay (``service: stays (SKEW)``) indented under it.  A variant that ends out of bound
    says which eligible domain is the lightest and what would give it room.  A report without variants is its note."""
    if not report.variants:
        return f"rebalance {report.stage}: {report.note or 'no variants'}"
    lines = []
    for i, v in enumerate(report.variants):
        lines.append(f"rebalance {v.name}: {len(v.moves)} services move ({v.moved_cpu_m}m cpu, {v.moved_mem_mib} MiB), "
                     f"skew over {report.spread_topology_key} {v.skew_before} -> {v.skew_after} "
                     f"(max_skew {report.spread_max_skew}), {v.n_stuck} attempts refused"
                     + (f", budget {v.max_moves}" if v.max_moves is not None else "")
                     + (" (best)" if i == report.best else ""))
        lines += [f"  {svc}: {src} -> {dst}" + (f" (relaxed: {', '.join(v.relaxed[svc])})" if v.relaxed.get(svc) else "")
                  for svc, src, dst in v.moves]
        lines += [f"  {svc}: stays ({why})" for svc, why in v.stuck.items()]
        if v.skew_after > (report.spread_max_skew or 0):
            lines.append(f"  still out of bound: {v.lightest} is the lightest eligible domain and takes no more of these "
                         "services; grow_stage(under_policy=True) says which servers would give it room")
    return "\n".join(lines)


def rebalance_report_to_dict(report: RebalanceReport) -> dict:
    d = {"stage": report.stage, "placement": {"strategy": report.strategy, "preferred": report.preferred},
         "pin": report.pin, "best": report.best,
         "plan": None if report.plan is None else json.loads(plan_to_json(report.plan)),
         "variants": [asdict(v) for v in report.variants]}
    if report.spread_topology_key is not None:
        d["placement"]["spread"] = {"topology_key": report.spread_topology_key, "max_skew": report.spread_max_skew}
    if report.fallback_relax_order:
        d["placement"]["fallback"] = {"relax_order": report.fallback_relax_order, "max_hops": report.fallback_max_hops}
    if report.note is not None:
        d["note"] = report.note
    return d


def rebalance_report_from_dict(d: dict) -> RebalanceReport:
    pol = d.get("placement") or {}
    variants = [RebalanceVariant(v["name"], list(v["order"]), [tuple(m) for m in v["moves"]], dict(v.get("stuck") or {}),
                                 {k: list(x) for k, x in (v.get("relaxed") or {}).items()}, v.get("n_stuck", 0),
                                 v.get("max_moves"), v.get("moved_cpu_m", 0), v.get("moved_mem_mib", 0),
                                 v.get("skew_before", 0), v.get("skew_after", 0), v.get("lightest"))
                for v in d.get("variants") or []]
    plan = d.get("plan")
    return RebalanceReport(d["stage"], pol.get("strategy"), list(pol.get("preferred") or []), list(d.get("pin") or []),
                           variants, d.get("best"),
                           None if plan is None else plan_from_json(json.dumps(plan, ensure_ascii=False)),
                           (pol.get("spread") or {}).get("topology_key"), (pol.get("spread") or {}).get("max_skew"),
                           list((pol.get("fallback") or {}).get("relax_order") or []),
                           (pol.get("fallback") or {}).get("max_hops"), d.get("note"))


def format_replan_report(report: Replan) -> str:
    """``replan <stage>: <k> kept, <n> new, <m> moved (<cpu>m cpu, <mem> MiB), <l> lost``, then the moves
    (``service: from -> to``), the new services (``service: -> to``) and the lost ones
    (``service: from -> lost (REASON)``) indented under it."""
    plan = report.plan
    lines = [f"replan {plan.stage}: {len(report.kept)} kept, {len(report.new)} new, {len(report.moved)} moved "
             f"({report.moved_cpu_m}m cpu, {report.moved_mem_mib} MiB), {len(report.lost)} lost"]
    lines += [f"  {svc}: {src} -> {dst}" for svc, src, dst in report.moved]
    lines += [f"  {svc}: -> {plan.assignment[svc]}" for svc in report.new]
    lines += [f"  {svc}: {src} -> lost ({why})" for svc, src, why in report.lost]
    # SPEC.md 2.14: what the kept seats alone leave outside the guarantees; printed only when set
    if report.skew_excess is not None:
        lines.append(f"  spread: skew {report.skew_excess} over {plan.spread_topology_key} exceeds max_skew "
                     f"{plan.spread_max_skew} (kept seats are not evicted)")
    if report.quota_over:
        lines.append(f"  quota: usage above the cap in {', '.join(report.quota_over)} (kept seats are not evicted)")
    return "\n".join(lines)


def replan_report_to_json(report: Replan, indent: int | None = None) -> str:
    """``{plan: <plan_to_json's object>, kept, new, moved, lost, moved_cpu_m, moved_mem_mib}``, and
    ``skew_excess`` / ``quota_over`` (SPEC.md 2.14) only when set."""
    d = {"plan": json.loads(plan_to_json(report.plan)), "kept": report.kept, "new": report.new,
         "moved": [list(m) for m in report.moved], "lost": [list(x) for x in report.lost],
         "moved_cpu_m": report.moved_cpu_m, "moved_mem_mib": report.moved_mem_mib}
    if report.skew_excess is not None:
        d["skew_excess"] = report.skew_excess
    if report.quota_over:
        d["quota_over"] = report.quota_over
    return json.dumps(d, ensure_ascii=False, indent=indent)


def replan_report_from_json(text: str) -> Replan:
    d = json.loads(text)
    return Replan(plan_from_json(json.dumps(d["plan"], ensure_ascii=False)), list(d.get("kept") or []),
                  list(d.get("new") or []), [tuple(m) for m in d.get("moved") or []],
                  [tuple(x) for x in d.get("lost") or []], d.get("moved_cpu_m", 0), d.get("moved_mem_mib", 0),
                  d.get("skew_excess"), list(d.get("quota_over") or []))


def format_grow_report(report: GrowReport) -> str:
    """One line per template, ``grow <name>: <opened> new servers take <placed> of <pending> services, <u> fit
    no such server, <c> over the cap of <max>``, with the services of each new server (``+<ordinal>: a, b``)
    indented under it where the candidate was detailed.  Under the policy (SPEC.md 2.18) the line goes on with
    ``; <n> on existing servers, <r> relaxed, <s> held by the skew, <q> by the quota`` and, under a constraint,
    `` [<key=value>: skew <before> -> <after>]``; the services that land on existing servers follow as
    ``service: -> server``, and a template without the topology key prints ``no candidate: no <key> label``."""
    lines = []
    for c in report.candidates:
        if report.under_policy and c.no_topology_key:
            lines.append(f"grow {c.name}: no candidate: no {report.spread_topology_key} label")
            continue
        line = (f"grow {c.name}: {c.opened} new servers take {c.placed} of {c.pending} services, "
                f"{c.unplaceable} fit no such server, {c.capped} over the cap of {c.max_new}")
        if report.under_policy:
            line += (f"; {c.on_live or 0} on existing servers, {len(c.relaxed)} relaxed, {c.stuck_skew or 0} held by the "
                     f"skew, {c.stuck_quota or 0} by the quota")
            if c.skew_before is not None:
                line += f" [{c.domain}: skew {c.skew_before} -> {c.skew_after}]"
        lines.append(line)
        lines += [f"  +{j}: {', '.join(svcs)}" for j, svcs in enumerate(c.servers or [])]
        lines += [f"  {svc}: -> {dst}" for svc, dst in c.moved_in]
    return "\n".join(lines)


# GrowCandidate's fields of SPEC.md 2.18: present in the JSON of a report made under the policy only
_GROW_POLICY_FIELDS = ("on_live", "relaxed", "stuck_skew", "stuck_quota", "skew_before", "skew_after", "domain", "moved_in",
                       "no_topology_key")


def grow_report_to_json(report: GrowReport, indent: int | None = None) -> str:
    """``{stage, max_new, pending, candidates}``; a report made under the policy (SPEC.md 2.18) adds
    ``placement`` (strategy, preferred, and spread / fallback / quota when set) and the candidates' policy fields."""
    cands = [asdict(c) for c in report.candidates]
    if not report.under_policy:
        for c in cands:
            for k in _GROW_POLICY_FIELDS:
                c.pop(k, None)
    d = {"stage": report.stage, "max_new": report.max_new, "pending": report.pending, "candidates": cands}
    if report.under_policy:
        pol = {"strategy": report.strategy, "preferred": report.preferred}
        if report.spread_topology_key is not None:
            pol["spread"] = {"topology_key": report.spread_topology_key, "max_skew": report.spread_max_skew}
        if report.fallback_relax_order:
            pol["fallback"] = {"relax_order": report.fallback_relax_order, "max_hops": report.fallback_max_hops}
        if report.quota is not None:
            pol["quota"] = {"caps": list(report.quota), "used": list(report.quota_used or (0, 0, 0))}
        d["placement"] = pol
    return json.dumps(d, ensure_ascii=False, indent=indent)


def grow_report_from_json(text: str) -> GrowReport:
    d = json.loads(text)
    cands = [GrowCandidate(**{**c, "labels": list(c["labels"]),
                              "servers": None if c.get("servers") is None else [list(s) for s in c["servers"]],
                              "relaxed": {k: list(v) for k, v in (c.get("relaxed") or {}).items()},
                              "moved_in": [tuple(m) for m in c.get("moved_in") or []]})
             for c in d.get("candidates") or []]
    report = GrowReport(d["stage"], d.get("max_new", 0), list(d.get("pending") or []), cands)
    pol = d.get("placement")
    if pol is not None:
        report.under_policy, report.strategy, report.preferred = True, pol.get("strategy"), list(pol.get("preferred") or [])
        report.spread_topology_key = (pol.get("spread") or {}).get("topology_key")
        report.spread_max_skew = (pol.get("spread") or {}).get("max_skew")
        report.fallback_relax_order = list((pol.get("fallback") or {}).get("relax_order") or [])
        report.fallback_max_hops = (pol.get("fallback") or {}).get("max_hops")
        if pol.get("quota") is not None:
            report.quota, report.quota_used = tuple(pol["quota"]["caps"]), tuple(pol["quota"]["used"])
    return report


def get_network_name(project: str, stage: str) -> str:
    """crates/fleetflow-container/src/converter.rs:12-14."""
    return f"{project}-{stage}"


def is_sensitive_key(key: str) -> bool:
    """crates/fleetflow/src/utils.rs:76-82."""
    k = key.lower()
    return "pass" in k or "secret" in k or "key" in k or "token" in k


def _service_block(flow: Flow, stage: str, name: str, container_suffix: str, plan: Plan | None) -> list[str]:
    svc = flow.services.get(name)
    if svc is None:
        raise FlowError(f"サービス '{name}' の定義が見つかりません")
    lines = ["", f"  サービス: {name}",
             f"    コンテナ: {flow.name}-{stage}-{name}{container_suffix}",
             f"    イメージ: {svc.image if svc.image is not None else '(未設定)'}"]
    for p in svc.ports:
        lines.append(f"    ポート: {p.host} → {p.container}/{p.protocol}")
    for v in svc.volumes:
        lines.append(f"    ボリューム: {v.host} → {v.container} ({'ro' if v.read_only else 'rw'})")
    if svc.environment:
        env = [f"{k}=***" if is_sensitive_key(k) else f"{k}={v}" for k, v in svc.environment.items()]
        lines.append(f"    環境変数: {', '.join(env)}")
    if plan is not None:
        lv = plan.levels.get(name)
        lines.append(f"    起動レベル: {'CYCLE' if lv == U32_MAX else lv}")
        if name in plan.candidates:  # stage 2: how many servers could take it on the pristine table
            cnt, first = plan.candidates[name]
            lines.append(f"    配置候補: {cnt} 台" + (f" (最初: {first})" if first else ""))
        if name in plan.assignment:
            relaxed = plan.relaxed.get(name)  # SPEC.md 2.8: placed after giving these label keys up
            lines.append(f"    配置先: {plan.assignment[name]}" + (f" (緩和: {', '.join(relaxed)})" if relaxed else ""))
        elif name in plan.rejected:
            lines.append(f"    配置先: (配置不可: {plan.rejected[name]})")
            if name in plan.quota_why:  # SPEC.md 2.10: the dimensions of the quota that refused it
                lines.append(f"    クォータ超過: {', '.join(plan.quota_why[name])}")
            if name in plan.why:
                lines.append(_why_line(plan.why[name]))
        else:
            lines.append("    配置先: local")
    return lines


def _why_line(w: Why) -> str:
    """The rejection diagnosis of one service (SPEC.md 2.9): the causes that fail somewhere, in the fixed
    order, with their server counts out of N (``全台`` marks one that fails on every server), then the
    required labels no schedulable server carries and the first server one cause away."""
    parts = [f"{c} {w.fail[c]}/{w.servers} 台" + (" (全台)" if c in w.universal else "")
             for c in WHY_NAMES if w.fail.get(c, 0) > 0]
    line = "    配置不可の理由: " + (", ".join(parts) if parts else "なし")
    notes = []
    if w.missing_labels:
        notes.append(f"該当ラベルなし: {', '.join(w.missing_labels)}")
    if w.nearest is not None:
        notes.append(f"最も近い: {w.nearest}")
    return line + (f" ({'; '.join(notes)})" if notes else "")


_FOOTER = "[dry-run] 実際の操作は行われません。--dry-run を外して実行してください。"


def _policy_lines(plan: Plan | None) -> list[str]:
    """The placement strategy (SPEC.md 2.6), the hard topology spread (2.7), the fallback chain (2.8) and
    the resource quota (2.10: use after the plan / cap, per capped dimension) a plan was made under; nothing
    without any."""
    if plan is None or (plan.strategy is None and not plan.preferred and plan.spread_topology_key is None
                        and not plan.fallback_relax_order and plan.quota is None):
        return []
    line = f"  配置戦略: {plan.strategy if plan.strategy is not None else 'first_fit'}"
    if plan.preferred:
        line += f" (優先ラベル: {', '.join(plan.preferred)})"
    lines = [line]
    if plan.spread_topology_key is not None:
        lines.append(f"  配置分散保証: {plan.spread_topology_key} (max_skew={plan.spread_max_skew})")
    if plan.fallback_relax_order:
        hops = "" if plan.fallback_max_hops is None else f" (max_hops={plan.fallback_max_hops})"
        lines.append(f"  配置フォールバック: {' → '.join(plan.fallback_relax_order)}{hops}")
    if plan.quota is not None:
        used = plan.quota_used if plan.quota_used is not None else (None,) * len(QUOTA_NAMES)
        parts = [f"{n} {'?' if u is None else u}/{c}" for n, c, u in zip(QUOTA_NAMES, plan.quota, used) if c is not None]
        lines.append(f"  配置クォータ: {', '.join(parts)}")
    return lines


def format_up_dry_run(flow: Flow, stage_name: str, plan: Plan | None = None) -> str:
    """up.rs:57-136 (``print_dry_run_plan``) over ``stage.services``."""
    stage = flow.stages[stage_name]
    lines = [f"[dry-run] ステージ '{stage_name}' の起動計画:", "",
             f"  ネットワーク: {get_network_name(flow.name, stage_name)} (作成予定)"]
    lines += _policy_lines(plan)
    for name in stage.services:
        lines += _service_block(flow, stage_name, name, "", plan)
    lines += ["", _FOOTER]
    return "\n".join(lines) + "\n"


def format_deploy_dry_run(flow: Flow, stage_name: str, target_services: list[str], tenant_line: str,
                          plan: Plan | None = None) -> str:
    """deploy.rs:14-100 (``print_dry_run_plan``) over the filtered target
    services; ``tenant_line`` is the already-resolved tenant description
    (deploy.rs:475-485)."""
    lines = [f"[dry-run] ステージ '{stage_name}' のデプロイ計画:", "", f"  テナント: {tenant_line}", "",
             f"  ネットワーク: {get_network_name(flow.name, stage_name)} (作成予定)"]
    lines += _policy_lines(plan)
    for name in target_services:
        lines += _service_block(flow, stage_name, name, " (停止・削除→再作成)", plan)
    lines += ["", _FOOTER]
    return "\n".join(lines) + "\n"


# ---- ordering consumers -------------------------------------

def start_waves(plan: Plan) -> list[list[str]]:
    """Parallel start waves for ``DeployEngine::create_and_start``
    (crates/fleetflow-container/src/engine.rs:355-452 starts services one by one in
    ``order_by_dependencies`` order).  Wave k holds the stage's services at level k
    in declaration order; every dependency of a wave-k service is in an earlier
    wave, so a wave's containers may be created and started concurrently (one
    ``join_all`` per wave).  Levels that no service has are skipped.  CYCLE
    services (level U32_MAX) are in no wave: the reference would start them in
    bucket 2 (engine.rs:83); the plan reports them in ``plan.rejected``."""
    by_level: dict[int, list[str]] = {}
    seen = set()
    for name in plan.level_order:
        lv = plan.levels[name]
        if lv == U32_MAX or name in seen:
            continue
        seen.add(name)
        by_level.setdefault(lv, []).append(name)
    return [by_level[k] for k in sorted(by_level)]


def unit_base_name(project: str, stage: str, service: str) -> str:
    """crates/fleetflow-container/src/quadlet.rs ``unit_base_name``: ``{project}-{stage}-{service}``."""
    return f"{project}-{stage}-{service}"


def quadlet_ordering_lines(project: str, stage: str, depends_on: list[str]) -> list[str]:
    """``[Unit]`` ordering of a generated ``.container`` unit, as the reference emits
    it (crates/fleetflow-container/src/quadlet.rs:95-100): for each dependency, in
    ``depends_on`` order, ``After=`` and ``Requires=`` on its generated service."""
    out = []
    for dep in depends_on:
        unit = f"{unit_base_name(project, stage, dep)}.service"
        out += [f"After={unit}", f"Requires={unit}"]
    return out


def compose_depends_on_lines(depends_on: list[str]) -> list[str]:
    """``depends_on:`` block of a compose service (crates/fleetflow-container/src/compose.rs:156-162);
    names are YAML-quoted by the reference only when they need it, which service
    names never do."""
    if not depends_on:
        return []
    return ["    depends_on:"] + [f"      - {d}" for d in depends_on]


def wave_start_script(plan: Plan, project: str) -> list[str]:
    """Human-readable start schedule: one line per wave with its containers
    (``{project}-{stage}-{service}``, up.rs:79 naming)."""
    return [f"  wave {i}: " + ", ".join(f"{project}-{plan.stage}-{s}" for s in wave)
            for i, wave in enumerate(start_waves(plan))]
