"""Shared by test_host_cpu.py and test_hip_forward.py: three small fully connected graphs and the workspace bytes of their plans at the default
configuration (8 heads, DIM_ATTEN 256, 2 layers, 160 / 26 classes, no feature transform, every switch of the handle at its default) with
32 points per object.  tests/plan_graph_check.cpp prints these numbers after holding the layout of csrc/plan_graph.h against the code
vlsat_plan_create had before it; the library must lay out the same plans."""

POINTS = 32
# (the name plan_graph_check.cpp prints, objects per scene, workspace bytes)
CASES = (("one scene of 9 nodes", (9,), 5411328),
         ("two scenes of 3 and 5 nodes", (3, 5), 2279424),
         ("one node, E = 0", (1,), 70144))
