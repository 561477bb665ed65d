"""fleetflow_amd -- MI355X-native placement planner for FleetFlow's plan path.

The product is libfleetplace.so (HIP, gfx950) behind include/fleetplace.h;
this package is its host-side mirror of the reference interface.
"""
from .planner import NONE, DevBatch, Planner  # noqa: F401
from .flow import (DrainReport, Flow, GrowCandidate, GrowReport, PlacementPolicy, Plan, RebalanceReport,  # noqa: F401
                   RebalanceVariant, Replan, Server, Service, ShrinkReport, ShrinkVariant, Stage, drain_stage, grow_stage,
                   order_by_dependencies, plan_stage, rebalance_stage, replan_stage, resolve_target_server, shrink_stage)
from .plan_output import (format_grow_report, format_rebalance_report, format_replan_report,  # noqa: F401
                          format_shrink_report, grow_report_to_json, rebalance_report_from_dict,
                          rebalance_report_to_dict, replan_report_to_json, shrink_report_to_json)
from .registry import plan_template  # noqa: F401

__all__ = ["NONE", "DevBatch", "Planner", "DrainReport", "Flow", "GrowCandidate", "GrowReport", "PlacementPolicy", "Plan",
           "RebalanceReport", "RebalanceVariant", "Replan", "Server", "Service", "ShrinkReport", "ShrinkVariant", "Stage", "drain_stage", "format_grow_report",
           "format_rebalance_report", "format_replan_report", "format_shrink_report", "grow_report_to_json", "grow_stage", "order_by_dependencies",
           "plan_stage", "plan_template", "rebalance_report_from_dict", "rebalance_report_to_dict", "rebalance_stage",
           "replan_report_to_json", "replan_stage", "resolve_target_server",
           "shrink_report_to_json", "shrink_stage"]
