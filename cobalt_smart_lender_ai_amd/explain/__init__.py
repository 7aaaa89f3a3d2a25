"""Model explanation: TreeSHAP explainer API, SHAP plots, partial dependence / ICE curves, permutation
importance."""
from .shap import (Explanation, TreeExplainer, bar_plot, force_data, importance_plot, partial_dependence, pd_plot,
                   permutation_importance, summary_plot, top_interactions)

__all__ = ["TreeExplainer", "Explanation", "bar_plot", "summary_plot", "force_data", "top_interactions",
           "partial_dependence", "pd_plot", "permutation_importance", "importance_plot"]
