"""A wave-level model of rt_descend_pop's control (ray-tracer_amd/csrc/rt_traverse.h) and of the macro step around it
(rt_render_loop.inc): 64 lanes in NumPy, no GPU and no HIP code - it tests the design.  The box and triangle tests are scripted per lane
(random enter / refuse outcomes, distances from a small set so that dist == best happens), the trees are random, with RT_REF_CHAIN edges and
empty leaves.  Checked, for every descend_keep in 0..64 and every entering lane count 1..64:
  - the loop ends, within (node visits + pops) iterations;
  - each lane's sequence of node visits, pops (taken or refused), triangle tests and mesh-done is the one of today's rt_descend + rt_pop, one
    macro step at a time, and its node visits and triangle tests are those tests/flat_emulator.py's FlatScene.mesh makes, in its order;
  - no lane touches a stack slot above stack_entries, or pops one that is not below its stack pointer (the loop reads the top of the stack
    together with the node, before it knows whether it will pop it: the model reads it at the same point, before the iteration's store)."""
import numpy as np
import pytest

import flat_emulator
from flat_emulator import FlatScene

LEAF, CHAIN, EMPTY, NODE_MASK = 0x80000000, 0x40000000, 0x80000000, 0x3FFFFFFF
INF = np.float32(1073741824.0)
WAVE = 64
DEPTH = 5                      # internal nodes on at most this many levels: stack_entries of the model's scene
EV_N, EV_P, EV_T, EV_D = 1 << 40, 2 << 40, 3 << 40, 4 << 40      # event codes: node visit | pop (the reference taken, EMPTY if refused) | triangle test | mesh done
POOL = 128                     # scripted rays (each with the root of the tree it walks)


class Model:
    """the scene (a few random trees in one node table) and the pool of scripted rays"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.lref, self.rref, self.roots, self.num_tris = [], [], [], 0

        def child(level):
            kind = rng.random()
            chain = CHAIN if rng.random() < 0.3 else 0
            if level < DEPTH and kind < (0.75 if level < 2 else 0.5):
                return chain | node(level)
            if kind < 0.9:
                count = int(rng.integers(1, 4))
                start, self.num_tris = self.num_tris, self.num_tris + count
                return LEAF | chain | (count << 20) | start
            return EMPTY

        def node(level):
            i = len(self.lref)
            self.lref.append(0), self.rref.append(0)
            self.lref[i], self.rref[i] = child(level + 1), child(level + 1)
            return i

        while len(self.roots) < 6:
            chain = CHAIN if rng.random() < 0.3 else 0
            self.roots.append(chain | node(1))
        self.lref, self.rref = np.array(self.lref, np.int64), np.array(self.rref, np.int64)
        n = len(self.lref)
        self.refs = np.stack([self.lref, self.rref], 1)
        self.root = np.array(self.roots, np.int64)[rng.integers(0, len(self.roots), POOL)]
        self.hit = rng.random((POOL, n, 2)) < 0.8
        self.dist = rng.integers(0, 6, (POOL, n, 2)).astype(np.float32)
        self.tri_hit = rng.random((POOL, self.num_tris)) < 0.7
        self.tri_t = rng.integers(1, 5, (POOL, self.num_tris)).astype(np.float32)
        self.today = [self.walk_today(r) for r in range(POOL)]

    # ---- one lane, today's code: rt_descend (to a leaf or a dead end), the leaf's triangles, rt_pop or mesh done, per macro step ----
    def walk_today(self, r):
        ev, stack, cur, best, prim = [], [], int(self.root[r]), INF, -1
        while True:
            while not cur & LEAF:
                ni = cur & NODE_MASK
                ev.append(EV_N | ni)
                ld, rd = self.dist[r, ni]
                l_push, r_push = bool(self.hit[r, ni, 0]) and ld < best, bool(self.hit[r, ni, 1]) and rd < best
                l_first = ld < rd
                if l_push and r_push:
                    stack.append((ld, int(self.lref[ni])) if l_first else (rd, int(self.rref[ni])))
                    cur = int(self.rref[ni] if l_first else self.lref[ni])
                elif l_push or r_push:
                    cur = int(self.lref[ni] if l_push else self.rref[ni])
                else:
                    cur = EMPTY
            for k in range((cur >> 20) & 1023):
                idx = (cur & 0xFFFFF) + k
                ev.append(EV_T | idx)
                if self.tri_hit[r, idx] and self.tri_t[r, idx] < best:
                    best, prim = self.tri_t[r, idx], idx
            if not stack:
                ev.append(EV_D)
                return np.array(ev, np.int64), best, prim
            dd, ref = stack.pop()
            cur = ref if dd < best or (dd == best and not ref & CHAIN) else EMPTY
            ev.append(EV_P | cur)


@pytest.fixture(scope="module")
def model():
    return Model(2024)


def test_todays_order_is_the_emulators(model, monkeypatch):
    """the per-lane order the wave model is held to is FlatScene.mesh's: same node visits, same triangle tests, same closest triangle"""
    n = len(model.lref)
    nodes = np.zeros((4 * n, 4), np.float32)
    for i in range(n):
        q = nodes[4 * i:4 * i + 4].reshape(16)
        q[0], q[6] = 2 * i, 2 * i + 1                     # the boxes carry (node, side): the scripted box test below reads them back
        q[12:14] = np.array([model.lref[i], model.rref[i]], np.uint32).view(np.float32)
    log = []

    def box_test(lo, hi, o, inv):
        key, r = int(lo[0]), int(o[0])
        if key < 0:
            return True, np.float32(0)                    # the root box: entered at distance 0
        if key % 2 == 0:
            log.append(EV_N | (key // 2))
        return bool(model.hit[r, key // 2, key % 2]), model.dist[r, key // 2, key % 2]

    def tri_test(tris, idx, o, d):
        log.append(EV_T | idx)
        return bool(model.tri_hit[int(o[0]), idx]), model.tri_t[int(o[0]), idx]

    monkeypatch.setattr(flat_emulator, "box_test", box_test)
    monkeypatch.setattr(flat_emulator, "tri_test", tri_test)
    fs = FlatScene.__new__(FlatScene)
    fs.nodes, fs.tris, fs.max_stack = nodes, None, 0
    refused = in_a_row = 0
    for r in range(POOL):
        del log[:]
        ob = {"v": np.array([-1, 0, 0, 0, 0, 0], np.float32), "root_ref": int(model.root[r])}
        o = np.array([r, 0, 0], np.float32)
        hit, best, prim = fs.mesh(ob, o, np.ones(3, np.float32), np.ones(3, np.float32))
        ev, t_best, t_prim = model.today[r]
        assert list(ev[(ev >> 40 == 1) | (ev >> 40 == 3)]) == log, r
        assert (best, prim) == (t_best, t_prim) and hit == (t_prim >= 0), r
        no = ev == (EV_P | EMPTY)
        refused += int(no.sum())
        in_a_row += int((no[1:] & no[:-1]).sum())
    assert fs.max_stack <= DEPTH
    # the inputs do contain what they are meant to: refused pops, and chains of consecutive ones
    assert refused > POOL // 2 and in_a_row >= 10, (refused, in_a_row)


def run_wave(model, rays, lanes, descend_keep):
    """The macro-step loop of rt_render_loop.inc for one wave whose `lanes` traverse with the scripted `rays` (the others hold no ray), with
    rt_descend_pop as the descend loop.  Returns per lane the event sequence and (best, prim), and the model's counters."""
    hit, dist, refs = model.hit, model.dist, model.refs
    ray = np.zeros(WAVE, np.int64)
    ray[lanes] = rays
    active = np.zeros(WAVE, bool)
    active[lanes] = True
    cur = np.where(active, model.root[ray], EMPTY)
    sp = np.zeros(WAVE, np.int64)
    best = np.full(WAVE, INF, np.float32)
    prim = np.full(WAVE, -1, np.int64)
    st_d = np.zeros((DEPTH + 1, WAVE), np.float32)
    st_r = np.zeros((DEPTH + 1, WAVE), np.int64)
    ev = np.zeros((WAVE, 256), np.int64)
    n_ev = np.zeros(WAVE, np.int64)
    all_lanes = np.arange(WAVE)
    budget = sum(int(((model.today[r][0] >> 40) <= 2).sum()) for r in rays)      # node visits + pops of the lanes, by today's code
    stats = {"loop_iterations": 0, "entered_on_empty": 0, "in_loop_pops": 0, "tie_on_chain": 0}

    def log(mask, code):
        i = all_lanes[mask]
        ev[i, n_ev[i]] = code[mask] if isinstance(code, np.ndarray) else code
        n_ev[i] += 1

    def pop(mask):
        """rt_pop for the lanes of `mask` (all have sp > 0)"""
        i = all_lanes[mask]
        sp[i] -= 1
        assert (sp[i] >= 0).all() and (sp[i] < DEPTH).all()              # a read: below the stack pointer it had, inside stack_entries
        dd, ref = st_d[sp[i], i], st_r[sp[i], i]
        stats["tie_on_chain"] += int(((dd == best[i]) & ((ref & CHAIN) != 0)).sum())
        take = (dd < best[i]) | ((dd == best[i]) & ((ref & CHAIN) == 0))
        cur[i] = np.where(take, ref, EMPTY)
        log(mask, EV_P | cur)

    def descend_pop(ex):
        # lanes that come in on the empty leaf pop until an entry is taken or their stack is empty; then only lanes on an internal node go on
        stats["entered_on_empty"] += int((ex & (cur == EMPTY)).sum())
        while True:
            again = ex & (cur == EMPTY) & (sp > 0)
            if not again.any():
                break
            stats["loop_iterations"] += 1
            assert stats["loop_iterations"] <= budget, "the entry pops do not end"
            stats["in_loop_pops"] += int(again.sum())
            pop(again)
        ex = ex & ((cur & LEAF) == 0)
        if not ex.any():
            return
        n_keep = (int(ex.sum()) * descend_keep) >> 6
        while True:
            stats["loop_iterations"] += 1
            assert stats["loop_iterations"] <= budget, "the loop does not end"
            assert (ex & ((cur & LEAF) != 0)).sum() == 0                 # every lane in the loop is on an internal node
            i = all_lanes[ex]
            # the top of the stack, read with the node and BEFORE this iteration's store (slot 0, unused, with an empty stack)
            top_slot = sp - (sp > 0)
            assert (top_slot[i] >= 0).all() and (top_slot[i] < DEPTH).all()
            top_d, top_r = st_d[top_slot, all_lanes], st_r[top_slot, all_lanes]
            ni = np.where(ex, cur & NODE_MASK, 0)
            log(ex, EV_N | ni)
            ld, rd = dist[ray, ni, 0], dist[ray, ni, 1]
            l_push = ex & hit[ray, ni, 0] & (ld < best)
            r_push = ex & hit[ray, ni, 1] & (rd < best)
            l_first = ld < rd
            both, entered = l_push & r_push, l_push | r_push
            assert (sp[i] <= DEPTH).all()                                # the store above the top: slot stack_entries at the most
            st_d[sp[i], i] = np.where(l_first, ld, rd)[i]
            st_r[sp[i], i] = np.where(l_first, refs[ni, 0], refs[ni, 1])[i]
            nxt = np.where(both, np.where(l_first, refs[ni, 1], refs[ni, 0]), np.where(l_push, refs[ni, 0], refs[ni, 1]))
            dead = ex & ~entered & (sp > 0)
            stats["in_loop_pops"] += int(dead.sum())
            stats["tie_on_chain"] += int((dead & (top_d == best) & ((top_r & CHAIN) != 0)).sum())
            take = (top_d < best) | ((top_d == best) & ((top_r & CHAIN) == 0))
            cur[ex] = np.where(entered, nxt, np.where(dead & take, top_r, EMPTY))[ex]
            sp[ex] = np.where(dead, top_slot, sp + both)[ex]
            log(dead, EV_P | cur)
            on_node = ex & ((cur & LEAF) == 0)
            stop = ex & ~on_node
            if int(on_node.sum()) < n_keep:
                stop = ex
            ex = ex & ~stop
            if not ex.any():
                return

    steps = 0
    while active.any():
        steps += 1
        assert steps <= budget + len(rays), "the macro steps do not end"
        enters = active & (((cur & LEAF) == 0) | ((cur == EMPTY) & (sp > 0)))
        if enters.any():
            descend_pop(enters)
        at_leaf = active & ((cur & LEAF) != 0)
        count = np.where(at_leaf, (cur >> 20) & 1023, 0)
        for k in range(int(count.max())):
            m = at_leaf & (k < count)
            idx = np.where(m, (cur & 0xFFFFF) + k, 0)
            log(m, EV_T | idx)
            closer = m & model.tri_hit[ray, idx] & (model.tri_t[ray, idx] < best)
            best[closer] = model.tri_t[ray, idx][closer]
            prim[closer] = idx[closer]
        popping = at_leaf & (sp > 0)
        if popping.any():
            pop(popping)
        done = at_leaf & ~popping
        log(done, EV_D)
        active &= ~done
    return ev, n_ev, best, prim, stats


def check_wave(model, rng, n_lanes, descend_keep, totals):
    lanes = np.sort(rng.choice(WAVE, n_lanes, replace=False))
    rays = rng.integers(0, POOL, n_lanes)
    ev, n_ev, best, prim, stats = run_wave(model, rays, lanes, descend_keep)
    for lane, r in zip(lanes, rays):
        want, w_best, w_prim = model.today[r]
        assert np.array_equal(ev[lane, :n_ev[lane]], want), (n_lanes, descend_keep, lane, r)
        assert (best[lane], prim[lane]) == (w_best, w_prim)
    idle = np.setdiff1d(np.arange(WAVE), lanes)
    assert (n_ev[idle] == 0).all()
    for k, v in stats.items():
        totals[k] = totals.get(k, 0) + v


@pytest.mark.parametrize("descend_keep", range(0, 65, 8))
def test_wave_model_every_keep_and_lane_count(model, descend_keep):
    """descend_keep in [k, k + 8) (0..64 over the cases) x every entering lane count 1..64"""
    rng = np.random.default_rng(1000 + descend_keep)
    totals = {}
    for keep in range(descend_keep, min(descend_keep + 8, 65)):
        for n_lanes in range(1, WAVE + 1):
            check_wave(model, rng, n_lanes, keep, totals)
    # what the cases are there for did happen: pops inside the loop, lanes that came in on the empty leaf with a stack, dist == best on a chain edge
    assert totals["in_loop_pops"] > 500 and totals["entered_on_empty"] > 50 and totals["tie_on_chain"] > 50, totals
