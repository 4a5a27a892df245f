"""TEST INFRASTRUCTURE of tests/test_gpu_move_forms.py, tests/test_move_forms_reference.py and tests/move_forms_worker.py: the one
scene all of them step (synthetic terrain, mixed crowd, everything but the skin stage), the sub-range plan, and the invariants
of the move stage's scheduling lists as `CharacterEngine.move_schedule()` reads them back from device memory."""
import numpy as np

from scenes import build_scene

TERRAIN = (32, 24)
LAND = 30                 # steps after which the crowd stands on the terrain (spawned 5 units above it: 19 steps of free fall)
DEFAULT_THRESHOLD = 4000  # sge_context_create's SGE_OPT_HEAVY_THRESHOLD
COST_CLASSES = 32         # classify_kernel / order_scatter_kernel: class = cost >> 7, clamped to 0..31

# (first, count) of every tick of one cycle of the sub-range case; (0, 0) is the whole crowd
RANGE_CROWD = 37
RANGE_PLAN = ((0, 0), (3, 5), (0, 16), (16, 21), (36, 1), (0, 0), (8, 9))
RANGE_CYCLES = 8          # per threshold


def stages(abi):
    return abi.STAGE_ALL & ~abi.STAGE_SKIN


def scene(pkg, eng, n, seed, agents=False):
    """The same crowd on either engine. With agents the spawn grid is drawn together (3 units between neighbours, capsules 3 wide)
    so that character-vs-character sweeps find somebody; every character keeps its 5 units of drop over the terrain."""
    _, terrain, state = build_scene(pkg, eng, n, terrain_cells=TERRAIN, seed=seed, mixed=True, rings=3, segments=3, agents=agents)
    if agents:
        b = state["bodies"].copy()
        span = max(float(np.abs(b["position"][:, [0, 2]]).max()), 1e-3)
        k = min(1.0, 1.5 * np.sqrt(n) / span)
        b["position"][:, 0] *= k
        b["position"][:, 2] *= k
        hx, hz = terrain["half"]
        b["position"][:, 1] = pkg.assets.terrain_height(b["position"][:, 0].astype(np.float64), b["position"][:, 2].astype(np.float64), hx, hz) + 2.5 + 5.0
        eng.upload(bodies=b)
    return state


def step(pkg, eng, first=0, count=0, exchange=None):
    """One tick of the case's stages on either engine. `exchange`: the product's parallel.AgentExchange when character-vs-character
    sweeps are on (the oracle then runs SGE_STAGE_AGENTS over all pairs)."""
    st = stages(pkg.abi)
    if getattr(eng.t, "is_product", False):
        if exchange is not None:
            exchange.step(stages=st)
        else:
            eng.tick(stages=st, first=first, count=count)
    else:
        import oracle_binding as ob
        ob.tick_mt(eng, 8, stages=st | (pkg.abi.STAGE_AGENTS if exchange is not None else 0), first=first, count=count)


def run_range_cycle(pkg, eng, plan=RANGE_PLAN):
    for first, count in plan:
        step(pkg, eng, first, count)


def landed(pkg, eng):
    g = eng.download(what=("controllers",))
    return float(((g["controllers"]["flags"] & pkg.abi.CTRL_GROUNDED_NEAR) != 0).mean())


def split_threshold(cost):
    """The median cost of the characters that cast at all: about half of them above it."""
    positive = np.asarray(cost)[np.asarray(cost) > 0]
    assert positive.size >= 2 and positive.min() < positive.max(), "a split needs two characters of different cost: %r" % (cost,)
    thr = int(np.median(positive))
    return thr if (positive > thr).any() else int(positive.min())


def cost_class(cost):
    return np.clip(np.asarray(cost, np.int64) >> 7, 0, COST_CLASSES - 1)


def check_schedule(sched, first, count, threshold, cost_before, tag=""):
    """The invariants of the lists in device memory behind a move stage over [first, first + count). `cost_before`: the range's
    costs of the step BEFORE the newest one (what lists that the newest stage built for itself were made from); None when the
    caller knows the lists were built for the next step."""
    counts, order, heavy = sched["counts"], sched["order"], sched["heavy"]
    assert sched["threshold"] == threshold, (tag, sched["threshold"], threshold)
    if sched["built_for_next"]:
        cost = sched["cost"]
    else:
        assert cost_before is not None, (tag, "lists of the newest stage itself: the costs they were built from are needed")
        cost = np.asarray(cost_before)
    assert cost.shape == (count,)
    assert int(counts[0]) + int(counts[1]) == count, (tag, counts)
    assert order.size == counts[0] and heavy.size == counts[1], (tag, counts)
    members = np.sort(np.concatenate([order, heavy]))
    assert np.array_equal(members, np.arange(first, first + count)), (tag, "heavy list + order list must hold every character of the range once", order, heavy)
    cls = cost_class(cost[order - first])
    assert (np.diff(cls) <= 0).all(), (tag, "the order list must not rise in cost class", cls)
    if threshold < 0:
        assert counts[1] == 0 and counts[2] == 0, (tag, counts)
    else:
        assert (cost[heavy - first] > threshold).all(), (tag, "a heavy-listed character at or under the threshold", cost[heavy - first], threshold)
        demand = int((cost > threshold).sum())
        assert counts[2] == demand and counts[1] == min(sched["cap"], demand), (tag, counts, demand, sched["cap"])
    assert counts[3] == int(np.maximum(cost, 0).sum()), (tag, counts, int(cost.sum()))
