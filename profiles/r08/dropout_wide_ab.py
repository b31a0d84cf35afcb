"""A/B of the dropout train loop for the wide addressing form: one run of profiles/r07/dropout_step.py's measurement (variant
fused p = 0.1, the three shapes of profiles/r07/dropout_step.txt) in THIS tree, optionally with gte_dropout_set_wide(1).

  python profiles/r08/dropout_wide_ab.py [--wide] [--steps 30] [--rounds 3]

The A/B of profiles/r08/dropout_wide_ab.txt alternates this script between a checkout of the parent commit (which runs
profiles/r07/dropout_step.py --only fused-0.1 itself: it has no hook) and this tree, on one box.
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    wide = "--wide" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--wide"]
    spec = importlib.util.spec_from_file_location("dropout_step", os.path.join(ROOT, "profiles", "r07", "dropout_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if wide:
        from gnn_tableextraction_amd import _lib
        _lib.check(_lib.load().gte_dropout_set_wide(1), "gte_dropout_set_wide")
    sys.argv = [sys.argv[0], "--only", "fused-0.1"] + argv
    print(f"# wide forced: {wide}")
    mod.main()


if __name__ == "__main__":
    main()
