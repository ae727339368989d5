"""Deterministic agronomic event schedules outside "one event a day, on tile position 0, the same on every site", and the
forcings that put a day's first record on other positions of the kernels' 16-step tile.

An event belongs to a (year, day) and falls on the first record of that day (events.c:470-482), so what a schedule reaches
depends on the forcing under it:

  daily2y       730 records of one day, 2021 and 2022: every record is a day's first, on any tile position; a record can
                carry events while both of its neighbours do
  lengths_3h    tests/forcing_regimes.py's 3-hour year: a day's first record on tile positions 0 and 8
  hh150_from1   the synthetic half-hourly year's first 150 days from record 1 on: a day's first record on tile position 15
  hh150_from15  the same from record 15 on: position 1

Each schedule is a function of the forcing's ClimTable and returns a list of sa.Event in file order (`k` below: the k-th day
of the file, from 0):

  same_record   day 20: all seven types, irrigation by both methods; day 45: two tillages (0.3 + 0.4); day 70: nine
                irrigations, canopy and soil alternating; day 100: a clear-cut (1, 1, 0, 0) and a planting
  first_last    all seven types on the file's first day and on its last
  consecutive   21 consecutive days from day 60 (+ shift) on, one event each, the seven types in turn
  tile_edges    days 15, 16, 31, 32, 33, 47, 64, 79, 95, 96: on daily2y the last record of a tile, the first of the next,
                both, and tiles left alone in between
  tillage       day 10: 0.005 (below the 0.01 threshold after its own step's decay: in effect during that step only);
                day 40: 0.02 (below the threshold after 21 decays of exp(-1/30)); day 100: 0.6, day 130: 0.3 while the first
                still decays (0.6 / e + 0.3 = 0.52), day 131: 0.4 on top of both (0.90: the stack above its largest member);
                and, where the forcing has a second year, 0.011 on its day 50 (three steps above the threshold)
  year_edge     all seven types on the last day of the first year and on the first day of the second
  per_site()    four sites of 730, 730, 400 and 611 daily records with four lists: same_record | none | consecutive shifted
                by 100 days | forty irrigations

Amounts are those of the suite's one-a-day schedule (tests/test_gpu_flags.py) where it has one.  Everything is generated here
from seeds; nothing is copied from any input file.  tests/test_event_regimes.py asserts the properties above and holds the
conditioning yardstick that lets tests/test_gpu_event_regimes.py use the fuzzer's bounds on these inputs."""
import numpy as np

import sipnet_amd as sa
from sipnet_amd import synth
from sipnet_amd.config import param_index as pi
from tests import forcing_regimes as fr
from tests import parameter_regimes as pr

FLAG_SETS = tuple(pr.FLAG_SETS)
FERT, HARVEST, IRRIG, PLANT, TILL, LEAFON, LEAFOFF = range(7)          # include/sipnet_amd.h
NAMES = {FERT: "fert", HARVEST: "harv", IRRIG: "irrig", PLANT: "plant", TILL: "till", LEAFON: "leafon", LEAFOFF: "leafoff"}
N_PARAMS = {FERT: 3, HARVEST: 4, IRRIG: 2, PLANT: 4, TILL: 1, LEAFON: 0, LEAFOFF: 0}
FORCINGS = ("daily2y", "lengths_3h", "hh150_from1", "hh150_from15")
TILE = 16
TILE_EDGE_DAYS = (15, 16, 31, 32, 33, 47, 64, 79, 95, 96)
CONSECUTIVE_FIRST, CONSECUTIVE_N = 60, 21
TILLAGE_DAYS = {"one_step": 10, "three_weeks": 40, "first": 100, "second": 130, "third": 131, "second_year": 365 + 50}
PER_SITE_LENGTHS = (730, 730, 400, 611)

# the amounts of tests/test_gpu_flags.py's schedule, by type
AMOUNTS = {FERT: (12.0, 40.0, 6.0), HARVEST: (0.2, 0.05, 0.3, 0.1), PLANT: (10.0, 30.0, 5.0, 8.0), TILL: (0.3,), LEAFON: (), LEAFOFF: ()}
IRRIG_CANOPY, IRRIG_SOIL = (2.5, 0), (1.5, 1)


def daily2y_raw(site=0, seed=fr.SEED):
    """730 records of one day, rounded like a file"""
    return synth.round_like_file(fr._by_lengths(np.full(730, 1.0), np.full(730, -86400.0), site, seed + 40))


def clim(name, site=0, gdd=1):
    if name == "daily2y":
        return synth.convert_raw(daily2y_raw(site), gdd)
    if name == "lengths_3h":
        return fr.clim("lengths_3h", site, gdd=gdd)
    first = {"hh150_from1": 1, "hh150_from15": 15}[name]
    whole = synth.convert_raw(synth.round_like_file(synth.half_hourly_year_raw(150 * 48, site=site)), gdd)
    return whole.slice(first, whole.n_steps)


def flags(flagset):
    return pr.flags(flagset)


def members(flagset="default"):
    """the 133 members of the regime tests (fr.hard_members) over the flag set's parameter file.  The default file's forest
    is evergreen (leafGrowth 0, fracLeafFall 0: a leaf-on or leaf-off event moves nothing), so every second member of that
    set is made deciduous as tests/state_edits.py does it; the other file is deciduous already"""
    out = fr.hard_members(pr.base(flagset))
    if flagset == "default":
        out[1::2, pi("leafGrowth")], out[1::2, pi("fracLeafFall")] = 60.0, 0.3
    return out


def day_starts(c):
    """the first record of every (year, day) of the forcing"""
    new = (c.day[1:] != c.day[:-1]) | (c.year[1:] != c.year[:-1])
    return np.flatnonzero(np.concatenate([[True], new]))


def event(c, k, typ, *p):
    """an event of type typ on the file's k-th day"""
    t = int(day_starts(c)[k])
    e = sa.Event()
    e.type, e.year, e.day = typ, int(c.year[t]), int(c.day[t])
    assert len(p) == N_PARAMS[typ]
    for i, v in enumerate(p):
        e.p[i] = float(v)
    return e


def of_type(c, k, typ, turn=0):
    """the suite's amounts; irrigation by the canopy on even turns, on the soil on odd ones"""
    return event(c, k, typ, *((IRRIG_SOIL if turn % 2 else IRRIG_CANOPY) if typ == IRRIG else AMOUNTS[typ]))


def all_types(c, k, both_methods=False):
    out = [of_type(c, k, typ) for typ in range(7)]
    if both_methods:
        out.insert(IRRIG + 1, of_type(c, k, IRRIG, 1))
    return out


def same_record(c):
    ev = all_types(c, 20, both_methods=True)
    ev += [event(c, 45, TILL, 0.3), event(c, 45, TILL, 0.4)]
    ev += [of_type(c, 70, IRRIG, i) for i in range(9)]
    ev += [event(c, 100, HARVEST, 1.0, 1.0, 0.0, 0.0), of_type(c, 100, PLANT)]
    return ev


def first_last(c):
    return all_types(c, 0) + all_types(c, len(day_starts(c)) - 1)


def consecutive(c, shift=0):
    return [of_type(c, CONSECUTIVE_FIRST + shift + i, i % 7, i // 7) for i in range(CONSECUTIVE_N)]


def tile_edges(c):
    return [of_type(c, k, i % 7, i // 7) for i, k in enumerate(TILE_EDGE_DAYS)]


def tillage(c):
    d = TILLAGE_DAYS
    ev = [event(c, d["one_step"], TILL, 0.005), event(c, d["three_weeks"], TILL, 0.02), event(c, d["first"], TILL, 0.6),
          event(c, d["second"], TILL, 0.3), event(c, d["third"], TILL, 0.4)]
    if len(day_starts(c)) > d["second_year"]:
        ev.append(event(c, d["second_year"], TILL, 0.011))
    return ev


def year_edge(c):
    k = int(np.argmax(c.year[day_starts(c)] != c.year[0]))           # the first day of the second year
    assert k > 0
    return all_types(c, k - 1) + all_types(c, k)


def forty_irrigations(c):
    return [of_type(c, 5 + 15 * i, IRRIG, i) for i in range(40)]


SCHEDULES = {"same_record": same_record, "first_last": first_last, "consecutive": consecutive, "tile_edges": tile_edges,
             "tillage": tillage, "year_edge": year_edge}
# the schedules that need one record a day or two years run on daily2y only
ANY_FORCING = ("same_record", "tillage")


def per_site():
    """-> (clims[4], events[4]): sites of different lengths and seeds with four different lists"""
    clims = [clim("daily2y", site=s).slice(0, n) for s, n in enumerate(PER_SITE_LENGTHS)]
    return clims, [same_record(clims[0]), [], consecutive(clims[2], shift=100), forty_irrigations(clims[3])]


def records_of(c, events):
    """the record every event falls on, by the reference's rule (events.c:470-482): the first whose year and day have both
    reached the event's"""
    out, t = [], 0
    for e in events:
        while t < c.n_steps and not (e.year <= c.year[t] and e.day <= c.day[t]):
            t += 1
        assert t < c.n_steps and (e.year, e.day) == (int(c.year[t]), int(c.day[t])), (e.year, e.day)
        out.append(t)
    return np.array(out, dtype=np.int64)


def copy_events(events):
    out = []
    for e in events:
        n = sa.Event()
        n.type, n.year, n.day = e.type, e.year, e.day
        for i in range(4):
            n.p[i] = e.p[i]
        out.append(n)
    return out


def moved(events, step):
    """the continuous amounts moved toward zero -- step(x) -> the neighbouring value; the exact constants 0 and 1 and the
    irrigation method held"""
    out = copy_events(events)
    for e in out:
        for i in range(N_PARAMS[e.type]):
            if not (e.type == IRRIG and i == 1) and e.p[i] not in (0.0, 1.0):
                e.p[i] = float(step(e.p[i]))
    return out


def events_in_text(events, without=()):
    """the list as an `events.in` (every amount with 17 significant digits: it reads back as the same double)"""
    lines = []
    for e in events:
        if e.type in without:
            continue
        p = [("%d" % int(e.p[i])) if (e.type == IRRIG and i == 1) else ("%.17g" % e.p[i]) for i in range(N_PARAMS[e.type])]
        lines.append(" ".join(["%d %d %s" % (e.year, e.day, NAMES[e.type])] + p))
    return "".join(ln + "\n" for ln in lines)
