"""fleetflow_amd -- MI355X-native placement planner for FleetFlow's plan path.

The product is libfleetplace.so (HIP, gfx950) behind include/fleetplace.h;
this package is its host-side mirror of the reference interface.
"""
from .planner import NONE, DevBatch, Planner  # noqa: F401
from .flow import (DrainReport, Flow, GrowCandidate, GrowReport, PlacementPolicy, Plan, Server, Service,  # noqa: F401
                   Stage, drain_stage, grow_stage, order_by_dependencies, plan_stage, resolve_target_server)
from .plan_output import format_grow_report, grow_report_to_json  # noqa: F401
from .registry import plan_template  # noqa: F401

__all__ = ["NONE", "DevBatch", "Planner", "DrainReport", "Flow", "GrowCandidate", "GrowReport", "PlacementPolicy", "Plan",
           "Server", "Service", "Stage", "drain_stage", "format_grow_report", "grow_report_to_json", "grow_stage",
           "order_by_dependencies", "plan_stage", "plan_template", "resolve_target_server"]
