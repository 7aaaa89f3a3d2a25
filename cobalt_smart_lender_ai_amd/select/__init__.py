from .collinearity import (CorrelationReport, Screen, correlation_matrix, drop_correlated,  # noqa: F401
                           vif)
