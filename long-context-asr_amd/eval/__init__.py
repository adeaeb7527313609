"""Evaluation: the loops of eval/run.py, the buffered and dynamic modes, WER, and context attribution.  The submodules are imported by
name; `context_attribution` (the function of the submodule of that name) and its result type are exported here on first use, so that
importing the package binds no ABI unit."""
import importlib


def __getattr__(name):
    if name in ('context_attribution', 'ContextAttribution'):
        m = importlib.import_module(__name__ + '.context_attribution')
        globals().update(context_attribution=m.context_attribution, ContextAttribution=m.ContextAttribution)
        return globals()[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
