"""Stage the reference's Python model package for tests/test_dropin_reference.py.

``build()`` copies ``<reference>/model/*.py`` into ``oracle/_ref/model/`` (git-ignored: nothing of the reference is
committed).  The reference checkout is taken from ``$LINA_REFERENCE_DIR``, else from ``/root/reference``; where neither
holds a readable ``model/`` package nothing is staged and the drop-in test skips.
"""
from __future__ import annotations

import glob
import os
import shutil

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
MODEL = os.path.join(OUT, "model")


def reference_dir() -> str:
    return os.environ.get("LINA_REFERENCE_DIR", "/root/reference")


def build() -> str | None:
    """Returns the staged directory (importable as ``model``), or None when no reference checkout is readable."""
    src = os.path.join(reference_dir(), "model")
    try:
        files = sorted(glob.glob(os.path.join(src, "*.py")))
        if not files:
            return None
        os.makedirs(MODEL, exist_ok=True)
        for f in files:
            shutil.copyfile(f, os.path.join(MODEL, os.path.basename(f)))
    except OSError:
        return None
    return MODEL
