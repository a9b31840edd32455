"""The launch vocabulary of csrc/whitted_params.h as the tests use it: the WT_F_* bits of a trace launch's flag word (read back with
clw_ext_last_trace_flags) and WT_SHAPE_FLAGS.  test_launch_plan_host.py reads the enum out of the header and holds this module to it."""
F_COUNT, F_DEEP, F_GEOM_LDS, F_RAYS, F_GRID, F_OCC, F_D8, F_D16, F_SHAPE = 1, 2, 4, 8, 16, 32, 64, 128, 256
F_SS, F_MOVE, F_LIST, F_ACC = 1 << 17, 1 << 18, 1 << 19, 1 << 20
SHAPE_MAX_SPHERES, SHAPE_MAX_PLANES, SHAPE_LIGHTS = 4, 2, 3


def shape_flags(ns, npl, nl=SHAPE_LIGHTS):
    """WT_SHAPE_FLAGS(ns, npl, nl): the shaped flavour stages its geometry in LDS and carries its counts in bits 9.."""
    return F_GEOM_LDS | F_SHAPE | ns << 9 | npl << 12 | nl << 14
