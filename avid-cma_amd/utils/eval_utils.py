"""``utils.eval_utils`` for a run of the reference's ``eval-action-recg.py`` / ``eval-action-recg-linear.py`` on this package: the reference's OWN module, executed
unmodified from wherever it lies on ``sys.path`` (``main_utils``' approach), with one name resolved differently.

``build_model`` (utils/eval_utils.py:332-343 of the reference) looks up the module-level name ``ClassificationWrapper`` when it is
CALLED; it is rebound here to ``models.classification.ClassificationWrapper`` — same constructor, ``state_dict`` and ``forward``,
and a training call through the stock tree runs as compiled launch programs (avid_hip/plan.py: ``ClsPlan``).  ``MOSTModel``
and ``Classifier`` (the linear probe, model ``MOSTWrapper``; utils/eval_utils.py:217-242, 298-329) are rebound the same way to
``models.linear_probe``: the heads' pooling, BatchNorm1d and Linear run on the kernels of csrc/probe.hip.  ``BatchWrapper``,
the checkpoint managers and the rest stay the reference's.  ``AVID_DROPIN=0`` leaves the module as it is.

Run the script through ``python -m avid_hip.run_reference eval-action-recg.py ...`` so that ``utils`` and ``models`` resolve
here first."""
import os as _os
import sys as _sys


def _reference_file():
    import utils as _pkg
    here = _os.path.dirname(_os.path.abspath(__file__))
    for d in list(_pkg.__path__) + [_os.path.join(p, "utils") for p in _sys.path if p]:
        f = _os.path.join(d, "eval_utils.py")
        if _os.path.isfile(f) and _os.path.abspath(d) != here:
            return f
    raise ImportError("utils.eval_utils: no eval_utils.py of the reference checkout on sys.path (put the AVID-CMA directory "
                      "behind avid-cma_amd on PYTHONPATH, or use python -m avid_hip.run_reference)")


REFERENCE_FILE = _reference_file()
with open(REFERENCE_FILE, "rb") as _f:
    exec(compile(_f.read(), REFERENCE_FILE, "exec"), globals())      # the reference's module body, in this namespace
DROPIN = _os.environ.get("AVID_DROPIN", "1") != "0"
if DROPIN:
    from models.classification import ClassificationWrapper  # noqa: E402,F811
    from models.linear_probe import MOSTModel, Classifier  # noqa: E402,F811
