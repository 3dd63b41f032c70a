"""The probes: rv_dev_math.h and orc_math.h behind one set of batch functions (build.py, inputs.py), and the narrow phase of
rv_dev_collide.h with the cross-lane primitives of rv_dev_wave.h behind another (build.py CollideProbe, collide_inputs.py)."""
