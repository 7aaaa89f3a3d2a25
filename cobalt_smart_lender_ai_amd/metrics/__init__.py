"""Model evaluation: ROC-AUC (``auc.py``), the classification report (``classification.py``) and bootstrap
confidence intervals with a paired model comparison (``bootstrap.py``)."""
from .bootstrap import BootstrapReport, bootstrap_ci

__all__ = ["BootstrapReport", "bootstrap_ci"]
