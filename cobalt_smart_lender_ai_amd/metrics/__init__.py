"""Model evaluation: ROC-AUC (``auc.py``), the classification report (``classification.py``), bootstrap
confidence intervals with a paired model comparison (``bootstrap.py``) and the calibration report
(``calibration.py``)."""
from .bootstrap import BootstrapReport, bootstrap_ci
from .calibration import ReliabilityReport, reliability_report

__all__ = ["BootstrapReport", "bootstrap_ci", "ReliabilityReport", "reliability_report"]
