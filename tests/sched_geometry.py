"""
The launch rules of the persistent scheduler kernels, mirrored in Python: forge_ec_amd/csrc/kernels.hpp (sched_grid,
wide_slots_pay) and cu_split.hpp (p256_cu_split).  The GPU tests read from here which kernel form a case takes, how many
fills of its slots a workgroup goes through and where the workgroups' ranges lie; tests/test_sched_launch_rules.py pins
every function below against the output of tests/cpp/sched_launch_rules.cpp, which calls the real ones.
"""
import collections

MAIN, WIDE = 864, 1024                      # QS_MAIN / PS_MAIN, QS_WIDE / PS_WIDE
VAR_MS, VAR_AFFINE_MS, FIXED_MS, FIXED_PREFIX_MS = 23.3, 20.9, 20.9, 19.1   # cu_split.hpp


def sched_grid(cus, n, cu_divisor=1):
    """(grid, per_wg) of a launch over n >= 1 elements for a ctx of `cus` CUs."""
    cus = cus or 256
    cap = cus // cu_divisor if cu_divisor > 1 and cus >= cu_divisor else cus
    grid = max(1, min(n // 64, cap))
    per_wg = (n + grid - 1) // grid
    return (n + per_wg - 1) // per_wg, per_wg


def wide_slots_pay(per_wg, main=MAIN, wide=WIDE):
    if per_wg <= main or per_wg > 3 * wide:
        return False

    def waste(q):
        return float(((per_wg + q - 1) // q) * q) / float(per_wg)
    return waste(wide) + 0.04 < waste(main)


def p256_cu_split(cus, n, var_ms, prefix_bits=0):
    """(CUs of the fixed-base launch, CUs of the variable-base launch beside it)."""
    cus = cus or 256
    f = FIXED_PREFIX_MS if prefix_bits >= 16 else FIXED_MS
    cf = int(float(cus) * f / (f + var_ms) + 0.5) if n >= 1 << 19 else cus // 2
    if cus % 8 == 0 and cus >= 16:
        cf = (cf + 4) // 8 * 8
        cf = min(max(cf, 8), cus - 8)
    cf = max(cf, 1)
    if cus > 1:
        cf = min(cf, cus - 1)
    return (cf, cus - cf) if cus > 1 else (cus, cus)


Shape = collections.namedtuple("Shape", "cus n grid per_wg wide slots fills ranges")


def shape(cus, n, fixed=False, cu_divisor=1):
    """The launch of p256_launch_mul / ed_launch_mul over n elements: `wide` the 1 024-slot instantiation (never for the
    P-256 fixed-base form), `fills` how often the fullest workgroup fills its slots (fills - 1 refills of every slot it
    keeps using), `ranges` the workgroups' [lo, hi)."""
    grid, per_wg = sched_grid(cus, n, cu_divisor)
    wide = (not fixed) and wide_slots_pay(per_wg)
    slots = WIDE if wide else MAIN
    ranges = [(w * per_wg, min(n, (w + 1) * per_wg)) for w in range(grid)]
    return Shape(cus, n, grid, per_wg, wide, slots, (per_wg + slots - 1) // slots, ranges)


def _pinned():
    pts = [(2, 1, n) for n in (1401, 2001, 3401, 4001, 5181, 7001)] + [(100, 1, 14901), (1, 1, 40037), (1, 1, 34037)]
    for n in (3000, (1 << 16) + 37):
        pts += [(c, 1, n) for c in (1, 2, 3, 4, 8, 16, 24, 32, 128)]          # whole ctx, and the shares p256_cu_split hands out
        pts += [(c, 2, n) for c in (1, 2, 3, 8, 16, 24, 32)]                  # Ed25519 beside its fixed-base launch
    pts += [(1, 1, 4096), (2, 1, 4096), (3, 1, 4096), (2, 1, 3500), (2, 1, 3501)]
    return sorted(set(pts))


# every (cus, cu_divisor, n) the GPU tests ask shape() about: tests/test_sched_launch_rules.py has the C++ program print
# exactly these and compares
PINNED = _pinned()
