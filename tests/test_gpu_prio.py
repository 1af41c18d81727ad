"""GPU: prioritised replay (PriorityTree; snac_prio_init / snac_prio_update / snac_prio_fill / snac_prio_sample, k_prio.hip) against the
numpy reference of tests/test_prio_host.py, and SelfPlay(prioritized=True) / ReplayRing(prioritized=True) on top of it.

Every comparison is exact: the weights are integers, the sums are uint64, and prob is one correctly rounded float64 division rounded
once to float32.  The tree's buffer is compared whole -- head, leaves, every level and all padding -- with the image the layout of
include/snac_hip.h ("Prioritised replay") gives for the reference's leaves.  Tree sizes 1, 65, 4097 and 262145 have 1, 2, 3 and 4 sum
levels, each with a ragged last group."""
import numpy as np
import pytest

from devmem import _env
import test_prio_host as ref
from test_gpu_uct_puct import make_evaluator

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 4097, 262145)
S = 16
SEED, SAMPLER = 0x1234567890ABCDEF, 11


def image(entries, w, max_weight):
    """The buffer's bytes for leaves w (uint32 [entries]): head, leaves, levels, zero padding."""
    nbytes, levels, off, _ = ref.layout(entries)
    buf = np.zeros(nbytes, np.uint8)
    buf[:24].view(np.uint64)[:] = (max_weight, entries, levels)
    buf[off[0]:off[0] + 4 * entries].view(np.uint32)[:] = w
    for l, sums in enumerate(ref.level_sums(w), 1):
        buf[off[l]:off[l] + 8 * len(sums)].view(np.uint64)[:] = sums
    assert l == levels and off[l] + 8 * len(sums) == nbytes
    return buf


def check_tree(tree, w, max_weight, what):
    got = tree.buffer.cpu().numpy()
    want = image(tree.entries, w, max_weight)
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d bytes differ, the first at byte %d (offsets %s)" % (what, len(bad), bad[0], tree.level_offset))


def _tree(entries, **kw):
    from snac_amd.priority import PriorityTree

    return PriorityTree(entries, "cuda:0", scale_log2=S, seed=SEED, sampler_id=SAMPLER, **kw)


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.asarray(a), dtype=dtype).to("cuda:0")


SPECIAL = np.float32([0.0, np.nan, -1.0, 1e-9, 1e9, 1.0, 0.5, 2.5 / 65536, np.inf, -0.0])


def make_priorities(rng, n):
    p = (rng.random(n) * 4.0).astype(np.float32)
    k = rng.random(n) < 0.4                                          # the special values, each of them for n >= 64
    p[k] = SPECIAL[rng.integers(0, len(SPECIAL), int(k.sum()))]
    p[:min(n, len(SPECIAL))] = SPECIAL[:min(n, len(SPECIAL))]
    return p


@pytest.mark.parametrize("entries", SIZES)
def test_init_update_and_fill_equal_the_reference(entries):
    import torch

    rng = np.random.default_rng(entries)
    tree = _tree(entries)
    assert (tree.bytes, tree.levels) == ref.layout(entries)[:2] and tree.levels == SIZES.index(entries) + 1
    w, mx = np.zeros(entries, np.uint32), 1 << S
    check_tree(tree, w, mx, "init")
    assert tree.weights().dtype == torch.uint32 and tuple(tree.weights().shape) == (entries,)
    assert tree.total() == 0 and tree.max_priority() == 1.0 and tree.head() == [1 << S, entries, tree.levels]
    for n in (1, 64, 65, 4096):
        idx = rng.integers(0, entries, n).astype(np.int32)
        if n >= 64:                                                  # out of range on both sides, and duplicates with different priorities
            idx[[3, 17, 40, 41]] = (-1, entries, -(1 << 31), (1 << 31) - 1)
            idx[50:56] = idx[20]
        p = make_priorities(rng, n)
        if n == 1:
            p[0] = 0.75
        tree.update(_dev(idx), _dev(p))
        mx = max(mx, ref.apply_update(w, idx.astype(np.int64), p, S))
        check_tree(tree, w, mx, "update n = %d" % n)
    assert mx == 0xFFFFFFFF and tree.max_priority() == 0xFFFFFFFF / 65536.0     # the clamp entered max_weight
    # duplicates: the largest weight wins wherever it stands in the batch, a zero among them included
    i, j = entries - 1, entries // 2
    idx = np.int32([i, i, i, j, j, j])
    p = np.float32([0.5, 2.0, 1.0, 0.0, 3.0, np.nan])
    tree.update(_dev(idx), _dev(p))
    ref.apply_update(w, idx.astype(np.int64), p, S)
    assert w[i] == (2 << S if i != j else 3 << S) and w[j] == 3 << S
    check_tree(tree, w, mx, "duplicates")
    tree.update(_dev(np.int32([j, j])), _dev(np.float32([0.0, 0.0])))            # and only zeros: the entry leaves the draw
    w[j] = 0
    check_tree(tree, w, mx, "zeros")
    tree.update(_dev(np.zeros(0, np.int32)), _dev(np.zeros(0, np.float32)))      # the empty job
    tree.update(_dev(np.int32([-5, entries])), _dev(np.float32([7.0, 9.0])))     # nothing in range: nothing changes, max_weight neither
    check_tree(tree, w, mx, "nothing in range")
    # fill: a single entry, a span across a 64- and a 4096-entry boundary (as far as the tree goes), the whole tree
    spans = [(entries - 1, 1), (min(50, entries - 1), min(4100, entries - min(50, entries - 1))), (0, entries)]
    for first, count in spans:
        for p, weight in ((0.25, 1 << (S - 2)), (None, mx), (0.0, 0), (1e6, 0xFFFFFFFF), (1e-9, 1)):
            tree.fill(first, count, p)
            w[first:first + count] = weight
            check_tree(tree, w, mx, "fill %d + %d with %r" % (first, count, p))  # max_weight follows update() only
    tree.fill(0, 0)
    check_tree(tree, w, mx, "the empty fill")
    assert tree.total() == int(w.sum(dtype=np.uint64))


def test_fill_reads_the_largest_weight_on_the_device():
    tree = _tree(200, )
    tree.fill(0, 100)                                                # before any update: priority 1.0
    w = np.zeros(200, np.uint32)
    w[:100] = 1 << S
    check_tree(tree, w, 1 << S, "fill before an update")
    tree.update(_dev(np.int32([150])), _dev(np.float32([0.5])))      # a smaller weight does not lower it
    w[150] = 1 << (S - 1)
    tree.fill(100, 10)
    w[100:110] = 1 << S
    check_tree(tree, w, 1 << S, "fill after a smaller update")
    tree.update(_dev(np.int32([151])), _dev(np.float32([2.5])))
    w[151] = 5 << (S - 1)
    tree.fill(110, 10)
    w[110:120] = 5 << (S - 1)
    check_tree(tree, w, 5 << (S - 1), "fill after a larger update")


def _weights_cases(entries, rng):
    """{name: uint32 leaves}.  Weights below 2^24 are set through update() with the exact float32 w / 2^16; 0xFFFFFFFF through 1e9."""
    mixed = rng.integers(0, 1 << 20, entries).astype(np.uint32)
    mixed[rng.random(entries) < 0.3] = 0
    mixed[rng.random(entries) < 0.05] = 0xFFFFFFFF
    few = np.zeros(entries, np.uint32)
    few[rng.integers(0, entries, 3)] = 1                             # T <= 3 < n: the q == 0 fallback
    last = np.zeros(entries, np.uint32)
    last[entries - 1] = 77
    cases = {"mixed": mixed, "few": few, "last": last, "empty": np.zeros(entries, np.uint32)}
    if entries > 400:
        run = rng.integers(1, 1000, entries).astype(np.uint32)
        run[entries // 2 - 100:entries // 2 + 100] = 0               # a zero run of 200 entries: more than three whole groups
        cases["run"] = run
    return cases


def _set(tree, w):
    import torch

    p = np.where(w == 0xFFFFFFFF, np.float32(1e9), (w.astype(np.float64) / 65536.0).astype(np.float32))
    assert ref.quant(p, S).tobytes() == w.tobytes()
    tree.update(torch.arange(tree.entries, device="cuda:0"), _dev(p.astype(np.float32)))


@pytest.mark.parametrize("entries", SIZES)
def test_sample_equals_the_reference(entries):
    rng = np.random.default_rng(100 + entries)
    tree = _tree(entries)
    seen = set()
    for name, w in _weights_cases(entries, rng).items():
        _set(tree, w)
        T = int(w.sum(dtype=np.uint64))
        assert tree.total() == T
        for n in (1, 7, 64, 1000):
            for stratified in (True, False):
                for draw in (0, 1, 5, (1 << 31) - 1):
                    tree.draw = draw
                    idx, prob, wt = tree.sample(n, stratified, with_weight=True)
                    assert tree.draw == draw + 1
                    want = ref.sample(w, n, SEED, SAMPLER, draw, stratified)
                    what = (name, n, stratified, draw)
                    assert idx.cpu().numpy().tobytes() == want[0].tobytes(), what
                    assert prob.cpu().numpy().tobytes() == want[1].tobytes(), what
                    assert wt.cpu().numpy().astype(np.uint32).tobytes() == want[2].tobytes(), what
                    if T:
                        assert (want[2] > 0).all() and want[0].min() >= 0 and want[0].max() < entries
                    else:
                        assert (want[0] == -1).all() and not want[1].any()
                    if name == "mixed" and n == 1000 and stratified:
                        seen.add(want[0].tobytes())
        if name == "mixed" and entries > 1:
            assert len(seen) == 4                                    # another draw, other entries
        if name == "mixed":                                          # the same draw again: the same entries
            tree.draw = 5
            a = tree.sample(64)
            tree.draw = 5
            b = tree.sample(64)
            assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    tree.draw = 9
    assert tuple(tree.sample(0)[0].shape) == (0,) and tree.draw == 10


def test_the_counter_stops_at_two_to_the_31_draws():
    tree = _tree(8)
    tree.draw = (1 << 31) - 1
    tree.sample(2)
    with pytest.raises(ValueError, match="2\\^31 times"):
        tree.sample(2)


# ---- the rings ------------------------------------------------------------------------------------------------------------------------
B, CAP, ITS = 4, 4, 2


def _selfplay(prioritized, moves=6):
    import torch

    from snac_amd import SelfPlay, UCTSearch

    env = _env(1, True, B, 21)
    search = UCTSearch(env, 16, 0, 0.97, c=1.25, paths=2, evaluator=make_evaluator(env.num_actions, False), max_iterations=(env.total_step + 1) * ITS)
    search.reset()
    play = SelfPlay(search, CAP, sample_moves=2, prioritized=prioritized)
    play.play(2, ITS)
    mid = None if play.tree is None else play.tree.weights().cpu().numpy().astype(np.int64)
    play.play(moves - 2, ITS)
    play.targets()
    torch.cuda.synchronize()
    return play, mid


def test_selfplay_gives_new_positions_the_largest_priority_and_play_is_undisturbed():
    import torch

    play, mid = _selfplay(True)
    assert play.tree.entries == CAP * B and play.tree.seed == play.env.seed
    assert mid.tolist() == [1 << S] * (2 * B) + [0] * (2 * B)        # after two moves: the written slots only
    assert play.tree.weights().cpu().numpy().tolist() == [1 << S] * (CAP * B)    # after six (wrapped): every entry
    assert play.tree.total() == (CAP * B) << S
    twin, _ = _selfplay(False)
    assert twin.tree is None
    for k in ("obs", "pi", "value", "action", "reward", "done", "move", "z"):
        assert torch.equal(getattr(play, k), getattr(twin, k)), k
    assert (play.head, play.moves) == (twin.head, twin.moves) and torch.equal(play.search.stats, twin.search.stats)
    with pytest.raises(ValueError, match="needs the priority tree"):
        twin.sample(4, prioritized=True)


def test_selfplay_samples_by_priority():
    import torch

    play, _ = _selfplay(True)
    n = CAP * B
    keep = torch.tensor([1, 6, 7, 12], device="cuda:0")
    pri = torch.zeros(n, device="cuda:0")
    pri[keep] = torch.tensor([0.5, 1.0, 2.0, 4.0], device="cuda:0")
    play.update_priorities(torch.arange(n, device="cuda:0"), pri)
    w = play.tree.weights().cpu().numpy().astype(np.uint32)
    assert np.flatnonzero(w).tolist() == keep.tolist()
    for stratified in (True, False):
        draw = play.tree.draw
        b = play.sample(1000, prioritized=True, beta=0.4, stratified=stratified)
        want = ref.sample(w, 1000, play.tree.seed, play.tree.sampler_id, draw, stratified)
        assert b["index"].dtype == torch.int64 and b["index"].cpu().numpy().tobytes() == want[0].tobytes()
        assert b["prob"].cpu().numpy().tobytes() == want[1].tobytes()
        assert set(b["index"].tolist()) == set(keep.tolist())        # entries of nonzero weight, and every one of them
        flat = b["index"]
        assert torch.equal(b["obs"], play.obs.view(n, -1)[flat].to(torch.float32)) and torch.equal(b["pi"], play.pi.view(n, -1)[flat])
        assert torch.equal(b["z"], play.z.view(-1)[flat]) and torch.equal(b["action"], play.action.view(-1)[flat].long())
        wt = (b["prob"] * float(len(play))) ** -0.4
        assert torch.equal(b["weight"], wt / wt.max()) and float(b["weight"].max()) == 1.0
        assert float(b["weight"].min()) < 1.0 and bool((b["weight"][flat == 1] == 1.0).all())      # the rarest entry weighs most
    ones = play.sample(64, prioritized=True, beta=0)["weight"]
    assert ones.tolist() == [1.0] * 64
    assert "index" not in play.sample(8)                             # the uniform path, as before
    play.play(1, ITS)                                                # the next move overwrites a slot: the largest priority seen (4.0)
    torch.cuda.synchronize()
    h = (play.head - 1) % CAP
    w2 = play.tree.weights().cpu().numpy().astype(np.int64)
    assert w2[h * B:(h + 1) * B].tolist() == [4 << S] * B
    rest = np.ones(n, bool)
    rest[h * B:(h + 1) * B] = False
    assert (w2[rest] == w.astype(np.int64)[rest]).all()


def test_reanalyse_draws_its_entries_from_the_tree():
    import torch

    from snac_amd import SelfPlay, UCTSearch

    env = _env(2, True, B, 22)
    fn = make_evaluator(env.num_actions, False)
    search = UCTSearch(env, 16, 0, 0.97, c=1.25, paths=2, evaluator=fn, max_iterations=(env.total_step + 1) * ITS)
    search.reset()
    play = SelfPlay(search, CAP, keep_states=True, prioritized=True)
    play.play(3, ITS)
    n = CAP * B
    pri = torch.zeros(n, device="cuda:0")
    pri[[2, 5, 9]] = torch.tensor([1.0, 1.0, 6.0], device="cuda:0")
    play.update_priorities(torch.arange(n, device="cuda:0"), pri)
    again = UCTSearch(env, 16, 0, 0.97, c=1.25, paths=2, evaluator=fn, max_iterations=4, trees=8)
    draw = play.tree.draw
    flat = play.reanalyse(again, 4, prioritized=True)
    torch.cuda.synchronize()
    want = np.sort(ref.sample(play.tree.weights().cpu().numpy(), 8, play.tree.seed, play.tree.sampler_id, draw, True)[0])
    want[1:][want[1:] == want[:-1]] = -1                             # eight draws of three entries: repeats, marked
    assert flat.cpu().numpy().tolist() == want.tolist() and (want == -1).sum() == 5
    refreshed = play.refreshed.view(-1).cpu().numpy()
    assert np.flatnonzero(refreshed).tolist() == [2, 5, 9] and refreshed.max() == 1


def test_replay_ring_keeps_the_predecessor_slot_out_of_the_draw():
    import torch

    from snac_amd import ReplayRing

    N, cap = 4, 4
    env = _env(2, True, N, 23)
    ring = ReplayRing(env, cap, prioritized=True)
    assert ring.tree.entries == cap * N and ring.tree.total() == 0
    ring.collect(2)
    assert ring.tree.weights().cpu().numpy().tolist() == [1 << S] * (2 * N) + [0] * (2 * N)      # before wrapping: the written slots
    b = ring.sample(64, prioritized=True)
    assert int(b["slot"].max()) <= 1 and int(b["slot"].min()) == 0
    ring.collect(3)                                                  # 5 ticks: wrapped, head = 1
    assert ring.head == 1 and ring.valid_ticks() == cap - 1
    w = ring.tree.weights().cpu().numpy().astype(np.uint32)
    assert w.reshape(cap, N).tolist() == [[1 << S] * N, [0] * N, [1 << S] * N, [1 << S] * N]
    draw = ring.tree.draw
    b = ring.sample(1000, prioritized=True, beta=0.5)
    want = ref.sample(w, 1000, ring.tree.seed, ring.tree.sampler_id, draw, True)
    assert b["index"].cpu().numpy().tobytes() == want[0].tobytes() and b["prob"].cpu().numpy().tobytes() == want[1].tobytes()
    assert torch.equal(b["index"], b["slot"] * N + b["env"]) and not bool((b["slot"] == ring.head).any())
    assert set(b["slot"].tolist()) == {0, 2, 3} and set(b["env"].tolist()) == set(range(N))
    g = ring.gather(b["slot"], b["env"])
    for k, t in g.items():
        assert torch.equal(b[k], t), k
    assert b["weight"].tolist() == [1.0] * 1000                      # equal priorities: equal weights
    # new priorities; the predecessor slot stays out although the caller names it
    idx = torch.arange(cap * N, device="cuda:0")
    ring.update_priorities(idx, (idx + 4).to(torch.float32) / 8.0)  # 0.5 .. 2.375
    w = ring.tree.weights().cpu().numpy().reshape(cap, N)
    assert not w[ring.head].any() and (w[[0, 2, 3]] > 0).all() and ring.tree.max_priority() == 2.375
    b = ring.sample(1000, prioritized=True)
    assert not bool((b["slot"] == ring.head).any()) and float(b["weight"].max()) == 1.0 and float(b["weight"].min()) < 1.0
    ring.collect(1)                                                  # slot 1 is written and drawable; slot 2 is the predecessor now
    w = ring.tree.weights().cpu().numpy().reshape(cap, N)
    assert w[1].tolist() == [19 << (S - 3)] * N and not w[2].any() and ring.head == 2
    assert "index" not in ring.sample(8)                             # the uniform path, as before


def test_the_tree_and_the_rings_never_synchronise_with_the_host():
    import torch

    from snac_amd import ReplayRing, SelfPlay, UCTSearch

    env = _env(2, True, B, 24)
    fn = make_evaluator(env.num_actions, False)
    search = UCTSearch(env, 16, 0, 0.97, c=1.25, paths=2, evaluator=fn, max_iterations=(env.total_step + 1) * ITS)
    search.reset()
    again = UCTSearch(env, 16, 0, 0.97, c=1.25, paths=2, evaluator=fn, max_iterations=ITS, trees=4)
    play = SelfPlay(search, CAP, keep_states=True, prioritized=True)
    renv = _env(2, True, B, 25)
    ring = ReplayRing(renv, CAP, prioritized=True)
    play.play(1, ITS)                                                # warm-up: every kernel and torch op of the window below
    play.targets()
    b = play.sample(8, prioritized=True)
    play.update_priorities(b["index"], (b["value"] - b["z"]).abs())
    play.reanalyse(again, ITS, prioritized=True)
    ring.collect(2)
    r = ring.sample(8, prioritized=True)
    ring.update_priorities(r["index"], r["reward"].abs())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        play.play(CAP, ITS)                                          # wraps
        play.targets()
        b = play.sample(8, prioritized=True, beta=0.5)
        play.update_priorities(b["index"], (b["value"] - b["z"]).abs())
        flat = play.reanalyse(again, ITS, prioritized=True)
        ring.collect(CAP)                                            # wraps: the span in two parts, the predecessor slot zeroed
        r = ring.sample(8, prioritized=True, stratified=False)
        ring.update_priorities(r["index"], r["reward"].abs())
        play.tree.fill(0, B, 0.5)
        i, p = play.tree.sample(5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(i.min()) >= 0 and float(p.sum()) > 0 and int(flat.max()) >= 0
    assert not bool((r["slot"] == ring.head).any()) and play.tree.draw == 5 and ring.tree.draw == 2
