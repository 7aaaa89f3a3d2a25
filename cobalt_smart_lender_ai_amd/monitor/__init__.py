"""Monitoring a deployed model: population-stability drift reports and WoE / IV tables (``drift.py``)."""
from .drift import (PSI_SHIFTED, PSI_STABLE, DriftAccumulator, DriftBaseline, DriftReport, bin_counts_host,
                    check_drift_edges, drift_cell, drift_edges, information_value, psi, psi_status, woe_iv)

__all__ = ["PSI_SHIFTED", "PSI_STABLE", "DriftAccumulator", "DriftBaseline", "DriftReport", "bin_counts_host",
           "check_drift_edges", "drift_cell", "drift_edges", "information_value", "psi", "psi_status", "woe_iv"]
