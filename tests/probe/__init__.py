"""The math probe: rv_dev_math.h and orc_math.h behind one set of batch functions (build.py, inputs.py)."""
