"""Models. ``Scorecard`` (``scorecard.py``) is exported lazily: it imports ``monitor.drift``, which imports
``models.sketch``."""


def __getattr__(name: str):
    if name == "Scorecard":
        from .scorecard import Scorecard

        return Scorecard
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["Scorecard"]
