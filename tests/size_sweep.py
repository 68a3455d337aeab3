"""Frame sizes and contents of the partial-CTU residue sweep (tests/test_size_sweep_cpu.py,
tests/test_gpu_size_sweep.py) -- a helper, not a test.

Everything the engine computes at a frame edge depends on W % 128, H % 128 and H % 32.  For
i = 1..31 let r = 4 i and s = 4 ((7 i) % 31 + 1): s runs through 4..124 as r does, in another
order, so every nonzero residue occurs exactly once per axis in each of the families A and B
(test_size_sweep_cpu.py test_every_residue_once_per_axis).  The tables are literals: a test
names the sizes it runs, whatever the formula."""
import numpy as np

from mipgpu.synth import synth_frame

# (128 + r, 128 + s): 2x2 CTUs -- one full CTU, a right-edge CTU, a bottom CTU and the corner
FAMILY_A = [
    (132, 160), (136, 188), (140, 216), (144, 244), (148, 148), (152, 176), (156, 204), (160, 232),
    (164, 136), (168, 164), (172, 192), (176, 220), (180, 248), (184, 152), (188, 180), (192, 208),
    (196, 236), (200, 140), (204, 168), (208, 196), (212, 224), (216, 252), (220, 156), (224, 184),
    (228, 212), (232, 240), (236, 144), (240, 172), (244, 200), (248, 228), (252, 132),
]
# (r, s) for odd i, (r, 128 + s) for even i: one CTU column narrower than 128 -- the 68-column
# quadrant window wraps over several frame rows
FAMILY_B = [
    (4, 32), (8, 188), (12, 88), (16, 244), (20, 20), (24, 176), (28, 76), (32, 232),
    (36, 8), (40, 164), (44, 64), (48, 220), (52, 120), (56, 152), (60, 52), (64, 208),
    (68, 108), (72, 140), (76, 40), (80, 196), (84, 96), (88, 252), (92, 28), (96, 184),
    (100, 84), (104, 240), (108, 16), (112, 172), (116, 72), (120, 228), (124, 4),
]
# residue 0 on one axis
FAMILY_C = [
    (256, 132), (256, 156), (256, 228), (256, 252),
    (132, 256), (188, 256), (196, 256), (252, 256),
]
ALL_SIZES = FAMILY_A + FAMILY_B + FAMILY_C

# the separable filters (samples above 1023 in the last columns at W % 128 != 0: the fixup
# kernel's CUs) and the 2-D ones, in the whitelist's order
SEP = ["filterFrame_1d_int", "filterFrame_1d_float", "filterFrame_1d_int_5x5", "filterFrame_1d_float_5x5"]
TWO_D = ["filterFrame_2d_int_quarterCtu", "filterFrame_2d_float_quarterCtu", "filterFrame_2d_int_5x5_quarterCtu",
         "filterFrame_2d_float_5x5_quarterCtu"]

CONTENTS = ("noise", "edges", "dark", "white")


def size_id(size):
    return "%dx%d" % size


def seed_of(w, h, salt=0):
    return 0x5E00 + 1000 * salt + 7 * w + h


def content(kind, w, h, salt=0):
    """A 10-bit frame.  noise: uniform (synth kind 1); edges: noise with columns 0..3 and
    W-4..W-1 at 1023 (the separable filters' last columns then exceed 1023 at every sweep size:
    the fixup path has something to do); dark: {0, 1, 2} (synth kind 2: filter quotients around
    1/2); white: all 1023 (the largest filter numerators)."""
    if kind == "noise":
        return synth_frame(w, h, seed_of(w, h, salt), 1)
    if kind == "edges":
        f = synth_frame(w, h, seed_of(w, h, salt), 1)
        f[:, :4] = 1023
        f[:, -4:] = 1023
        return f
    if kind == "dark":
        return synth_frame(w, h, seed_of(w, h, salt), 2)
    if kind == "white":
        return np.full((h, w), 1023, np.uint16)
    raise ValueError(kind)


def caller_refs(w, h, salt=0):
    """Caller-supplied reference frame: noise; where W % 128 != 0 the columns W-2 and W-1 hold
    values in [1024, 1705] (the range of the reference's separable filters there), which the
    input contract allows in those two columns (their CUs go to the exact per-CU kernel)."""
    r = synth_frame(w, h, seed_of(w, h, salt) ^ 0xCA11, 1)
    if w % 128:
        hi = np.random.default_rng(seed_of(w, h, salt)).integers(1024, 1706, (h, 2))
        r[:, -2:] = hi.astype(np.uint16)
    return r
