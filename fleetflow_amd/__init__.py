"""fleetflow_amd -- MI355X-native placement planner for FleetFlow's plan path.

The product is libfleetplace.so (HIP, gfx950) behind include/fleetplace.h;
this package is its host-side mirror of the reference interface.
"""
from .planner import NONE, DevBatch, Planner  # noqa: F401
from .flow import (DrainReport, Flow, GrowCandidate, GrowReport, PlacementPolicy, Plan, Replan, Server,  # noqa: F401
                   Service, ShrinkReport, ShrinkVariant, Stage, drain_stage, grow_stage, order_by_dependencies, plan_stage, replan_stage,
                   resolve_target_server, shrink_stage)
from .plan_output import (format_grow_report, format_replan_report, format_shrink_report, grow_report_to_json,  # noqa: F401
                          replan_report_to_json, shrink_report_to_json)
from .registry import plan_template  # noqa: F401

__all__ = ["NONE", "DevBatch", "Planner", "DrainReport", "Flow", "GrowCandidate", "GrowReport", "PlacementPolicy", "Plan",
           "Replan", "Server", "Service", "ShrinkReport", "ShrinkVariant", "Stage", "drain_stage", "format_grow_report",
           "format_replan_report", "format_shrink_report", "grow_report_to_json", "grow_stage", "order_by_dependencies",
           "plan_stage", "plan_template", "replan_report_to_json", "replan_stage", "resolve_target_server",
           "shrink_report_to_json", "shrink_stage"]
