"""Deterministic member sets far from the one perturbed forest of synth.perturbed_params.

The throughput kernels rewrite the reference's expressions of the PARAMETERS once per member (reciprocals, log2 of the
Q10s, exp2 of their products, 1 / ((psnTMax - psnTMin) / 2)^2 ...), narrow the results to float in fp32-mixed batches,
choose template instantiations by two exponents and branches by a dozen more values, and let one member's state decide
which tile path its 63 neighbours take.  The regimes below put members where those rewrites, preconditions and branches
can go wrong.  The ranges are the `min max` columns of tests/golden/smoke/niwot/sipnet.param, parsed here: 77 of its
rows have max > min, and 55 of those name a parameter of the 80-value vector this model carries (the other 22 belong to
the microbe, quality and cold-soil structures, which neither this project nor the reference's Params struct has).

  wide        133 members; every ranged parameter uniform over its range.  The allocations are a Dirichlet draw over the
              four (so the derived coarse-root allocation is >= 0 and every member valid), fineRootFrac + coarseRootFrac
              <= 0.9 (the wood pool starts positive).  dVpdExp and soilRespMoistEffect are random: the general-exponent
              instantiations.  The same draw under every flag set: the oracle runs all of it (status 0, finite
              planes) under the nitrogen-cycle flags too, where several members' wood pools run to exactly 0
  wide_plain  the same draw with dVpdExp = 2 and soilRespMoistEffect = 1 exactly: the plain-exponent instantiations
  corners     154 members; the base with ONE ranged parameter at its minimum (member 2k) or maximum (member 2k + 1) for
              the 55 ranged parameters, then 44 members with TWO different parameters at an extreme each.
              leafAllocation and woodAllocation at their maxima are invalid (status 3) and stay in the set
  edges       133 members; hand-picked exact values (edge_values), one or two per member, at lanes 0, 63, 64, 127, in the
              ragged chunk and between; the rest is synth.perturbed_params(scale=3).  Preconditions of the reference
              that the set keeps on purpose: the allocation one ulp past the last valid one and leafAllocation 1 are
              refused (status 3, lanes 63 and 64); under the nitrogen-cycle flags soilInit 0 and litterInit 0 (lanes
              127 and 132) make the reference itself non-finite -- it divides by the empty pool -- so their values
              are judged nowhere, their status and their neighbours are; and fAnoxia 1, clamped to 1 - 1e-6, makes it
              divide by 1e-6 (AMPLIFIED below)
  crop        133 members around the raw vector of tests/golden/smoke/russell_1|2|3/sipnet.param: member 0 is the file,
              the others have the synth.PERTURB parameters multiplied by exp(N(0, 0.15)).  laiInit 0, an aMax beyond
              niwot's range, dVpdExp 1.43, day-of-year phenology with leaf growth and fall

Everything is generated from seeds and from fixtures already in the tree.  tests/test_parameter_regimes.py asserts the
properties above and holds the conditioning yardstick that lets tests/test_gpu_parameter_regimes.py use the fuzzer's
tight bounds on these members.
"""
import os

import numpy as np

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DATA = os.path.join(REPO, "sipnet_amd", "data")
NIWOT = os.path.join(HERE, "golden", "smoke", "niwot", "sipnet.param")
SEED = 20261019

NCYCLE_FLAGS = dict(litterPool=1, anaerobic=1, nitrogenCycle=1)
RUSSELL_3 = dict(growthResp=1, leafWater=1, litterPool=1, waterHResp=0)
FLAG_SETS = {"default": {}, "ncycle": NCYCLE_FLAGS, "russell_3": RUSSELL_3}
CROP_CASES = {"crop_1": ("russell_1", ("default",)), "crop_2": ("russell_2", ("default", "ncycle")),
              "crop_3": ("russell_3", ("default", "russell_3"))}
SYNTHETIC = ("wide", "wide_plain", "corners", "edges")
REGIMES = SYNTHETIC + tuple(CROP_CASES)

# parameters the model compares with forcing values or dates: moving one across an equality is another input, not a rounding
COMPARED = ("leafOnDay", "leafOffDay", "gddLeafOn", "soilTempLeafOn", "frozenSoilThreshold", "coldSoilThreshold")
ALLOCATIONS = ("leafAllocation", "woodAllocation", "fineRootAllocation")
ROOT_FRACS = ("fineRootFrac", "coarseRootFrac")
Q10S = ("vegRespQ10", "soilRespQ10", "fineRootQ10", "coarseRootQ10")


def flags(flagset):
    return sa.flags_from(**FLAG_SETS[flagset])


def base(flagset):
    path = os.path.join(DATA, "base_forest.param" if flagset == "default" else "allflags_forest.param")
    return sa.read_params(path, flags(flagset))[0]


def ranges():
    """name -> (min, max) of the fixture's rows with max > min that name a parameter of the vector, in file order"""
    out = {}
    with open(NIWOT) as fh:
        for line in fh:
            tok = line.split("!")[0].split()
            if len(tok) >= 5 and pi(tok[0]) >= 0 and float(tok[4]) > float(tok[3]):
                out[tok[0]] = (float(tok[3]), float(tok[4]))
    return out


def wide(base_vec, n=133, plain=False, seed=SEED):
    rng = np.random.default_rng(seed)
    out = np.tile(np.asarray(base_vec, dtype=np.float64), (n, 1))
    for name, (lo, hi) in ranges().items():
        out[:, pi(name)] = rng.uniform(lo, hi, n)           # (drawn for every name, so that the streams below do not move)
    alloc = rng.dirichlet(np.ones(4), n)                    # leaf, wood, fine root, (coarse root: derived)
    for k, name in enumerate(ALLOCATIONS):
        out[:, pi(name)] = alloc[:, k]
    first = rng.uniform(0.0, 0.9, n)                        # one fraction over [0, 0.9], the other over what it leaves
    second = rng.uniform(0.0, 1.0, n) * (0.9 - first)
    swap = rng.random(n) < 0.5
    roots = np.stack([np.where(swap, second, first), np.where(swap, first, second)], axis=1)
    for k, name in enumerate(ROOT_FRACS):
        out[:, pi(name)] = roots[:, k]
    if plain:
        out[:, pi("dVpdExp")] = 2.0
        out[:, pi("soilRespMoistEffect")] = 1.0
    return out


N_DOUBLE_CORNERS = 44


def corner_table():
    """[(member, ((name, value), ...))]: single corners in file order, then the double corners"""
    rg = ranges()
    names = list(rg)
    table = []
    for k, name in enumerate(names):
        table.append((2 * k, ((name, rg[name][0]),)))
        table.append((2 * k + 1, ((name, rg[name][1]),)))
    rng = np.random.default_rng(SEED + 1)
    safe = [n for n in names if n not in ALLOCATIONS]       # (an allocation at its maximum is invalid: singles only)
    for j in range(N_DOUBLE_CORNERS):
        a, b = rng.choice(len(safe), 2, replace=False)
        ea, eb = rng.integers(0, 2, 2)
        table.append((2 * len(names) + j, ((safe[a], rg[safe[a]][ea]), (safe[b], rg[safe[b]][eb]))))
    return table


def corners(base_vec):
    table = corner_table()
    out = np.tile(np.asarray(base_vec, dtype=np.float64), (len(table), 1))
    for m, pairs in table:
        for name, v in pairs:
            out[m, pi(name)] = v
    return out


def exact_fine_root_allocation(vec):
    """1 - leaf - wood as the model's setup computes the remainder in double: the coarse-root allocation is then
    (1 - leaf - wood) - that, exactly 0 -- the last valid value"""
    return 1.0 - vec[pi("leafAllocation")] - vec[pi("woodAllocation")]


# the lanes that matter most first: chunk starts and ends, the ragged chunk
EDGE_LANES_FIRST = (0, 63, 64, 127, 128, 132)


def edge_values(flagset):
    """the hand-picked members, as dicts name -> value (or a function of the member's own vector)"""
    one_up = np.nextafter(1.0, 2.0)
    e = [
        {"laiInit": 0.0},                                                       # lane 0
        {"fineRootAllocation": lambda v: np.nextafter(exact_fine_root_allocation(v), 2.0)},   # lane 63: invalid by one ulp
        {"leafAllocation": 1.0},                                                # lane 64: invalid
        {"soilInit": 0.0},                                                      # lane 127
        {"plantWoodInit": 0.0},                                                 # lane 128
        {"litterInit": 0.0},                                                    # lane 132
        {"fineRootAllocation": exact_fine_root_allocation},                     # the last valid value
        {"soilWFracInit": 0.0}, {"soilWFracInit": 1.0},
    ]
    for q in Q10S:
        e += [{q: 1.0}, {q: one_up}]
    e += [
        {"psnTMin": lambda v: v[pi("psnTOpt")] - 0.5},
        {"aMax": 0.0}, {"baseFolRespFrac": 0.0}, {"attenuation": 1e-6}, {"halfSatPar": 0.01},
        {"immedEvapFrac": 0.0}, {"immedEvapFrac": 1.0}, {"fastFlowFrac": 0.0}, {"fastFlowFrac": 1.0},
        {"waterRemoveFrac": 0.0}, {"waterRemoveFrac": 1.0},
        {"snowMelt": 0.0}, {"frozenSoilEff": 0.0, "frozenSoilThreshold": 5.0},
        {"wueConst": 0.01}, {"wueConst": 109.0}, {"soilWHC": 0.1}, {"rdConst": 0.0},
        {"dVpdExp": 1.0}, {"dVpdExp": 3.0}, {"soilRespMoistEffect": 0.0}, {"soilRespMoistEffect": 2.5},
        {"snowInit": 50.0}, {"leafTurnoverRate": 1.0, "woodTurnoverRate": 1.0},
    ]
    if flagset != "default":
        e += [
            {"fAnoxia": 0.0}, {"fAnoxia": 1.0}, {"anaerobicDecompRate": 0.0}, {"anaerobicDecompRate": 1.5},
            {"nFixationFracMax": 1.0}, {"anaerobicTransExp": 2.0}, {"anaerobicTransExp": 2.5},
            {"mineralNInit": 0.0}, {"soilOrgNInit": 0.0}, {"litterOrgNInit": 0.0}, {"plantStorageNInit": 0.0},
            {"soilCSaturation": lambda v: v[pi("soilInit")]},
        ]
    return e


def edge_lanes(n_edges, n=133):
    rest = [m for m in range(n) if m not in EDGE_LANES_FIRST][1::2]
    lanes = list(EDGE_LANES_FIRST) + rest
    assert n_edges <= len(lanes)
    return lanes[:n_edges]


def edges(base_vec, flagset="default", n=133):
    """-> (members, table): table = [(lane, {name: value})] with the values as set"""
    out = synth.perturbed_params(base_vec, n, scale=3.0)
    values = edge_values(flagset)
    table = []
    for lane, spec in zip(edge_lanes(len(values), n), values):
        done = {}
        for name, v in spec.items():
            done[name] = float(v(out[lane])) if callable(v) else float(v)
            out[lane, pi(name)] = done[name]
        table.append((lane, done))
    return out, table


def crop_base(case, flagset):
    path = os.path.join(HERE, "golden", "smoke", case, "sipnet.param")
    return sa.read_params(path, flags(flagset))[0]


def crop(base_vec, n=133, seed=SEED + 2):
    rng = np.random.default_rng(seed)
    out = np.tile(np.asarray(base_vec, dtype=np.float64), (n, 1))
    for name in synth.PERTURB:
        f = np.exp(rng.normal(0.0, 0.15, n))
        f[0] = 1.0
        out[:, pi(name)] *= f
    return out


def regime_base(regime, flagset):
    if regime in CROP_CASES:
        return crop_base(CROP_CASES[regime][0], flagset)
    return base(flagset)


def members(regime, flagset="default"):
    b = regime_base(regime, flagset)
    if regime == "wide":
        return wide(b)
    if regime == "wide_plain":
        return wide(b, plain=True)
    if regime == "corners":
        return corners(b)
    if regime == "edges":
        return edges(b, flagset)[0]
    return crop(b)


def flag_sets_of(regime):
    return CROP_CASES[regime][1] if regime in CROP_CASES else tuple(FLAG_SETS)


def clim(site=0):
    """one year of the synthetic climate, rounded like a file"""
    return synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(17520, site=site)))


def continuous_columns(regime):
    """[(column, target)]: the parameters the yardstick moves, and where to: the middle of the range -- for `crop`,
    whose values lie outside niwot's ranges, the PERTURB parameters toward the base value (target None)"""
    if regime in CROP_CASES:
        return [(pi(n), None) for n in synth.PERTURB if n not in COMPARED]
    return [(pi(n), 0.5 * (lo + hi)) for n, (lo, hi) in ranges().items() if n not in COMPARED]


def held(regime, flagset, mem):
    """[members][80] bool: values the yardstick leaves as they are.  In `edges` a hand-set value IS the test (an exact
    0, 1.0 or one ulp above it, the last valid allocation): moving it is another input, not a rounding -- and where
    the edge is an allocation, the edge is on the sum of the three, so all three stay"""
    hold = np.zeros(mem.shape, dtype=bool)
    if regime == "edges":
        for lane, spec in edges(base(flagset), flagset)[1]:
            names = set(spec) | (set(ALLOCATIONS) if set(spec) & set(ALLOCATIONS) else set())
            for name in names:
                hold[lane, pi(name)] = True
    return hold


# Members the narrowed proxy of tests/test_parameter_regimes.py moves by more than 1e-4 of the plane maximum, by name:
# left out of the fp32-mixed comparison of VALUES only (their status is judged; fp64 judges all of them).
#   corners, fineRootAllocation at its maximum 0.6: with leaf and wood at 0.2 the coarse-root allocation is
#   1 - 0.2 - 0.2 - 0.6, a rounding residue above 0 -- the edge of validity; 0.6 rounded to float is above it (status 3)
F32_PROXY_EXCLUDED = {"corners": (("fineRootAllocation", 1),)}

# Members whose one-ulp move the REFERENCE amplifies beyond the 1e-12 yardstick, by name, with the bar they are held to:
#   edges (flag sets with the anaerobic flag), fAnoxia 1: setup clamps it to 1 - 1e-6 and the model divides by
#   1 - fAnoxia = 1e-6, so one ulp in soilWHC or soilWFracInit is 1e6 ulps in the anaerobic index.  Held to 1e-11: a
#   hundredth of the GPU bound instead of a thousandth.  The same factor -- 5e-12 for one double ulp, 5e4 ulps of the
#   plane maximum -- turns ONE fp32 rounding (6e-8) of the soil's water fraction, which an fp32-mixed kernel makes on
#   every step, into 3e-3 of the plane maximum: the ramp of the anaerobic index is 1e-6 of the water fraction wide,
#   17 float steps.  So this member is left out of the fp32-mixed comparison of values too; the CPU test asserts that
#   it is the only one whose one-ulp figure, scaled from a double's ulp to a float's, exceeds 1e-4
AMPLIFIED = {"edges": (("fAnoxia", 1.0, 1e-11),)}


def f32_proxy_excluded(regime):
    """member indices of F32_PROXY_EXCLUDED"""
    out = []
    for name, end in F32_PROXY_EXCLUDED.get(regime, ()):
        out += [m for m, pairs in corner_table() if len(pairs) == 1 and pairs[0] == (name, ranges()[name][end])]
    return out


def f32_excluded(regime, flagset):
    """the members left out of the fp32-mixed comparison of values: the narrowed proxy's and the amplified ones"""
    return sorted(set(f32_proxy_excluded(regime)) | set(amplified(regime, flagset)))


def amplified(regime, flagset):
    """{member: bar} of AMPLIFIED"""
    out = {}
    if regime == "edges":
        for lane, spec in edges(base(flagset), flagset)[1]:
            for name, value, bar in AMPLIFIED["edges"]:
                if spec.get(name) == value and FLAG_SETS[flagset].get("anaerobic"):
                    out[lane] = bar
    return out
