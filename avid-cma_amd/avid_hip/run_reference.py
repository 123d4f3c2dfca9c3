"""``python -m avid_hip.run_reference SCRIPT [args...]``: run one of the reference's scripts (``main-avid.py``,
``eval-action-recg.py``) as ``__main__`` with this package's directory AHEAD of the script's own.

``python SCRIPT`` puts the script's directory first on ``sys.path``, so ``utils``, ``models`` and ``utils.main_utils`` would
resolve to the reference checkout's and this package would not be imported at all.  Here the order is: this package
(``avid-cma_amd``), the script's directory, then the rest of ``sys.path`` — ``models`` is this package's, ``utils`` spans both
directories (utils/__init__.py), and ``utils.main_utils`` / ``utils.eval_utils`` execute the reference's own files with
this package's pieces bound in."""
import os
import runpy
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        sys.stderr.write("usage: python -m avid_hip.run_reference SCRIPT [args...]\n")
        return 2
    script = os.path.abspath(argv[0])
    sdir = os.path.dirname(script)
    rest = [p for p in sys.path if p and os.path.abspath(p) not in (PKG, sdir)]
    sys.path[:] = [PKG, sdir] + rest
    sys.argv = [script] + argv[1:]
    runpy.run_path(script, run_name="__main__")
    return 0


if __name__ == "__main__":
    sys.exit(main())
