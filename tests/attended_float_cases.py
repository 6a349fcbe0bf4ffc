"""Inputs of test_gpu_attended_float.py (qmann_hops_top_float_i8 / qmann_hops_shared_top_float_i8, csrc/hops_attended_float.h),
shared with the CPU preconditions in test_attended_float_inputs.py.

SHARED cases are shared_float_cases cases: ONE memory of S slots and B questions, carried as a float_hops_cases.Case whose planes
are the memory repeated B times.  Both new calls run on every one of them -- the shared call on the memory, the per-story call on
the copies -- so every family below reaches both selections.  STORY cases are float_hops_cases cases for what only the per-story
call has: empty stories, mixed lengths in one batch, a batch cut by max_slots, rows no query owns.

Ordinary cases inherit the generator's spread conditions (float_hops_cases.py: three quarters of the (query, hop) rows with
S >= 8 have 1 / sum p^2 >= 4), and on top of them test_attended_float_inputs.py asserts that in at least DISTINCT_SHARE of those
(query, hop) rows the first min(17, S) probabilities of the reference, as floats, are pairwise distinct: there the order is
decided by the values alone and a selection that loses or repeats a slot shows.  Seeds that miss it are replaced in SEEDS.

The tie families do not depend on u, so they tie in every hop whatever the read-out's last bit does:
  mirrored   row s + S / 2 equals row s in keys and values: every probability occurs twice, every odd k cuts a pair;
  constant   all rows equal: all p equal, the answer is slots 0 .. k - 1;
  zero_scale att_scale = 0: the same through the scale layer;
  underflow  att_scale = 10^4: e^x underflows to 0 everywhere but at the maxima, the zeros fill up by lowest slot;
  nan        the shift-based normaliser on top of that: the total is below sqrt 2, llrint(log2 total) = 0, the maxima get
             1 / 0 = +inf and every other slot 0 / 0 = NaN -- so a NaN probability IS reachable in mode 1 (the CPU reference
             shows it: test_attended_float_inputs.py), and it ranks below every number, by lowest slot among themselves.
             One hop: the state behind a NaN read-out has no reference.
"""
from functools import lru_cache

import numpy as np

import float_hops_cases as fc
import shared_float_cases as sf
from float_hops_cases import pad_dim, tile_edge_slots, tile_rows

KS = (1, 5, 16)
TILES = sf.TILES
BATCHES = sf.BATCHES
CAP_SLOTS = sf.CAP_SLOTS
SLOT_COUNTS = (1, 4, 5, 6, 15, 16, 17, 255, 256, 257)
DISTINCT_SHARE = 0.75            # the share float_hops_cases guarantees for its spread condition
DISTINCT_PLACES = 17             # places 1 .. 16 and the first one left out
# name -> seed, where the default (a hash of the name) failed a condition (here always: the share of distinct first places)
SEEDS = {"af_s256": 9101, "af_s257": 9100, "af_d128_s129": 9100, "af_d128_s385": 9102, "af_d60_s256": 9101, "af_d60_s513": 9101,
         "af_d60_s575": 9100, "af_d60_s769": 9102}
# Cases whose scores repeat among the first places by themselves -- 38 368 or 4 097 scores on one integer grid, or the coarse grids
# of the three format draws -- so that fewer rows than DISTINCT_SHARE have distinct first places under the default seed and under each
# of twelve others (9100 .. 9111).  They stay: the yardstick orders their ties like any others; they are not counted as ordinary.
GRID_TIES = ("af_cap", "af_s4097", "af_formats_00", "af_formats_01", "af_formats_02")
TIE_FAMILIES = ("mirrored", "constant", "zero_scale", "underflow", "nan")
BIG_SCALE = 1.0e4


# ---- special memories ---------------------------------------------------------------------------------------------------------------
def _mirror(rng, case):
    S = case.kb.shape[1]
    assert S % 2 == 0
    case.kb[:, S // 2:] = case.kb[:, :S // 2]
    case.vb[:, S // 2:] = case.vb[:, :S // 2]
    case.marks["mirrored"] = S // 2


def _constant(rng, case):
    case.kb[:, 1:] = case.kb[:, :1]
    case.vb[:, 1:] = case.vb[:, :1]
    case.marks["constant"] = True


SHARED = {}
STORY = {}


def _shared(name, family, **kw):
    assert name not in SHARED and name not in sf.CASES and name not in fc.CASES
    SHARED[name] = dict(family=family, **kw)


def _story(name, family, **kw):
    assert name not in STORY and name not in fc.CASES
    STORY[name] = dict(family=family, **kw)


# slot counts around k = 5 and 16 and around one 256-thread pass of the selection
for _S in SLOT_COUNTS:
    _shared(f"af_s{_S}", "slots", D=60, S=_S, B=5)
# tile edges of both scans at every padded width
for _D in (60, 128, 200):
    for _S in tile_edge_slots(pad_dim(_D)):
        _shared(f"af_d{_D}_s{_S}", "tile_edges", D=_D, S=_S, B=5)
_shared("af_s4097", "slots", D=60, S=4097, B=3)
_shared("af_cap", "cap", D=60, S=CAP_SLOTS, B=2)                 # one memory at the cap: every thread holds 150 slots
# every batch size under every forced tile: full tiles, a short last tile of one query and of three
_T = tile_rows(64)
for _B in BATCHES:
    _shared(f"af_batch_{_B:02d}", "batches", D=60, S=_T + 1, B=_B)
# ties
_shared("af_mirrored_130", "mirrored", D=60, S=130, B=5, special=_mirror)
_shared("af_mirrored_600", "mirrored", D=128, S=600, B=3, special=_mirror)
_shared("af_constant_97", "constant", D=60, S=97, B=5, special=_constant)
_shared("af_constant_300", "constant", D=200, S=300, B=3, special=_constant)
_shared("af_zero_scale", "zero_scale", D=60, S=150, B=5, tune="none", cfg_extra=dict(att_scale=[0.0, 0.0, 0.0]))
_shared("af_underflow", "underflow", D=60, S=150, B=5, tune="none", cfg_extra=dict(att_scale=[BIG_SCALE] * 3))
_shared("af_underflow_pow2", "underflow", D=60, S=300, B=3, tune="none", cfg_extra=dict(att_scale=[BIG_SCALE] * 3, softmax_variant=1))
_shared("af_nan", "nan", D=60, S=150, B=5, H=1, tune="none",
        cfg_extra=dict(att_scale=[BIG_SCALE], softmax_variant=0, softmax_shift_based=True))
# switches
_shared("af_scale_negative", "switches", D=60, S=150, B=5, scale_signs=[-1, 1, -1])
_shared("af_pow2", "switches", D=60, S=150, B=5, cfg_extra=dict(softmax_variant=1))
_shared("af_plan", "switches", D=60, S=150, B=5, cfg_extra=dict(softmax_variant=2))
_shared("af_shift_pow2", "switches", D=60, S=150, B=5, cfg_extra=dict(softmax_variant=1, softmax_shift_based=True))
_shared("af_shift_exp", "switches", D=128, S=150, B=5, cfg_extra=dict(softmax_variant=0, softmax_shift_based=True))
_shared("af_no_lin_map", "switches", D=128, S=150, B=5, en_lin_map=False)
_shared("af_binary_relu", "switches", D=60, S=150, B=5, fmt_bin=(0, 0), cfg_extra=dict(en_non_lin=True))
for _i in (0, 1, 2):
    _a, _w, _t, _bn = fc.rand_formats(_i)
    _shared(f"af_formats_{_i:02d}", "switches", D=(60, 128, 200)[_i % 3], S=70, B=5, fmt=_a, fmt_w=_w, fmt_att=_t, fmt_bin=_bn)
_shared("af_tied", "tied", D=100, S=129, B=7, tied=True)

# the per-story call alone
_story("afs_mixed", "mixed", D=60, S_in=[0, 1, 5, 17, 64, 65, 300, 16, 0, 257])
_story("afs_mixed_d128", "mixed", D=128, S_in=[33, 0, 4, 129, 6, 15])
_story("afs_cut", "cut", D=60, S_in=[10, 200, 90, 400], max_slots=100)
_story("afs_cut_to_3", "cut", D=60, S_in=[2, 3, 4, 70], max_slots=3)
_story("afs_lead_rows", "mixed", D=200, S_in=[40, 7, 66], lead_rows=9)
_story("afs_tied", "tied", D=60, S_in=[20, 0, 131], tied=True)


def _seeded(name, make, *args, **kw):
    """the generators seed from a hash of the name; a replaced seed goes in through their SEEDS tables"""
    if name in SEEDS:
        sf.SEEDS[name] = fc.SEEDS[name] = SEEDS[name]
    return make(name, *args, **kw)


@lru_cache(maxsize=None)
def build(name):
    if name in SHARED:
        spec = dict(SHARED[name])
        return _seeded(name, sf._make, spec.pop("family"), **spec)
    spec = dict(STORY[name])
    return _seeded(name, fc._make, spec.pop("family"), **spec)


def family(name):
    return (SHARED.get(name) or STORY[name])["family"]


def ordinary(name):
    """decided by value: not a tie family and not in GRID_TIES"""
    return family(name) not in TIE_FAMILIES and name not in GRID_TIES


@lru_cache(maxsize=None)
def reference_p(name):
    """[query][hop] -> the reference's probabilities as float32 (the nan case: its one hop)"""
    case = build(name)
    out = []
    for q in range(case.B):
        u, hops = case.u0[q], []
        for h in range(case.cfg["n_hop"]):
            hp = case.hop(q, h, u)
            hops.append(hp.p.astype(np.float32))
            if h + 1 < case.cfg["n_hop"]:
                u = hp.u_next_f32()
        out.append(hops)
    return out


def distinct_share(name):
    """share of the (query, hop) rows with S >= 8 -- the rows the generator tunes and gives its guarantee for; shorter stories keep
    their raw score scale and underflow -- whose first min(DISTINCT_PLACES, S) reference probabilities are pairwise distinct floats"""
    ok = []
    for hops in reference_p(name):
        for p in hops:
            if p.size < fc.SPREAD_MIN_SLOTS:
                continue
            first = np.sort(p)[::-1][:DISTINCT_PLACES]
            ok.append(len(set(first.tolist())) == first.size)
    return float(np.mean(ok)) if ok else 1.0
