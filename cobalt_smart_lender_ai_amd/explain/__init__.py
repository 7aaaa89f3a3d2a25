"""Model explanation: TreeSHAP explainer API (path-dependent and interventional), SHAP plots, partial dependence /
ICE curves, accumulated local effects, permutation importance, counterfactual recourse, integrated gradients of the
MLP challenger."""
from .nn import MLPExplainer
from .recourse import RecourseReport, counterfactuals
from .shap import (FEATURE_PERTURBATIONS, Explanation, TreeExplainer, accumulated_local_effects, ale_plot, bar_plot,
                   force_data, importance_plot, partial_dependence, pd_plot, permutation_importance, summary_plot,
                   top_interactions)

__all__ = ["TreeExplainer", "Explanation", "FEATURE_PERTURBATIONS", "bar_plot", "summary_plot", "force_data",
           "top_interactions", "partial_dependence", "pd_plot", "accumulated_local_effects", "ale_plot",
           "permutation_importance", "importance_plot", "counterfactuals", "RecourseReport", "MLPExplainer"]
