"""Every entry of the evaluation caches, read back from the device and checked against the C oracle (tests/cachecheck.py).

The cross-tree table (cz_search_set_xcache) is shared by all trees of a context and filled by many waves of one launch at once.
Here 4096 trees file into ONE bucket of 64 entries (or four), so that claims, lost swaps and replacements of a full bucket happen
in every launch; after every expand_backup launch the whole table is read back and every entry must be one position's: its
board, key and bucket, its ordered legal labels with their (src, dst), the priors and the value its expansion gives — bit for
bit — and no key may still carry the reserved "being written" bit.  The trees themselves must stay the oracle's.  The per-tree
entries, which follow their nodes through both re-rooting kernels, are checked against the trees after every advance."""
import numpy as np
import pytest
import torch

import cachecheck as CC
import fakenet
from conftest import open_boards

pytestmark = pytest.mark.gpu

G, PLAYOUTS, PLIES, CAP = 4096, 64, 2, 24000
XC_FROM_STEP = 3


def _roots():
    """Distinct root positions: the start position, its 44 successors (black to move), second-ply positions (red to move),
    third-ply positions (black to move) and open boards with up to 110 legal moves (either side)."""
    from oracle import oracle as O
    b0 = O.fen_to_board(O.START_FEN)
    pos = [(b0, 0)]
    succ = [O.apply_move(b0, int(m))[0] for m in O.legal_moves(b0, 0)]
    pos += [(b, 1) for b in succ]
    for b1 in succ[::11]:
        for m in O.legal_moves(b1, 1)[:24]:
            b2 = O.apply_move(b1, int(m))[0]
            pos.append((b2, 0))
            pos.append((O.apply_move(b2, int(O.legal_moves(b2, 0)[int(m) % 7]))[0], 1))
    ob, os_ = open_boards(48, 31)
    pos += [(ob[i], int(os_[i])) for i in range(len(ob))]
    return np.stack([p[0] for p in pos]), np.array([p[1] for p in pos], np.uint8)


def _played(st):
    """The most visited root child (ties: the first), like get_action with temperature -> 0."""
    n = st["N"].astype(np.int64).copy()
    n[np.arange(128)[None, :] >= st["count"].astype(np.int64)[:, None]] = -1
    played = st["label"][np.arange(len(n)), n.argmax(axis=1)].astype(np.uint16)
    played[st["count"] == 0] = 0xFFFF
    return played


@pytest.fixture(scope="module")
def oracle_run():
    """The oracle's plain schedule on the DISTINCT roots (tree g of the device run is root g % D): per ply root statistics,
    status and tree dumps."""
    from oracle import oracle as O
    boards, side = _roots()
    D = len(boards)
    fwd = fakenet.make_forward("signed", 5)
    orc = O.Search(D, CAP)
    orc.reset(boards, side, np.zeros(D, np.int32))
    out = []
    for ply in range(PLIES):
        for step in range(PLAYOUTS + 1):
            op, _ = orc.select(0 if step == 0 else 1)
            orc.expand_backup(*fwd(op))
        st = orc.root_stats()
        out.append((st, orc.status()[0].copy(), [orc.tree_dump(d) for d in range(D)]))
        orc.advance(_played(st))
    return boards, side, out


@pytest.mark.parametrize("log2_entries,key_bits,adv_global", [(6, 64, 0), (8, 64, 1), (6, 11, 0), (6, 11, 1)])
def test_contended_xcache_entries_are_whole_positions(oracle_run, log2_entries, key_bits, adv_global):
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import SearchEngine
    boards, side, ostates = oracle_run
    D = len(boards)
    idx = np.arange(G) % D                  # every root filed by ~G / D trees, spread over all workgroups and XCDs
    mask = CC.key_mask(key_bits)
    fwd = fakenet.make_forward("signed", 5)
    ref = CC.Reference(CC.oracle_expander(fwd))
    eng = SearchEngine(G, CAP)
    h = eng.ctx.h
    check(lib().cz_search_debug_eval_cache_key_bits(h, key_bits), "cz_search_debug_eval_cache_key_bits")
    check(lib().cz_search_debug_advance_in_global_memory(h, adv_global), "cz_search_debug_advance_in_global_memory")
    try:
        eng.set_eval_cache(True)
        eng.reset(boards[idx], side[idx], np.zeros(G, np.int32))
        filings, launches, dups, ec_checked = [], 0, 0, 0
        for ply in range(PLIES):
            eng.set_terminal_extra(4)
            eng.set_sim_target(PLAYOUTS)
            for step, mode in enumerate([0] + [1] * PLAYOUTS):
                if ply == 0 and step == XC_FROM_STEP:
                    # the table starts empty a few lock-steps into the search: the first filings are then leaves of several
                    # depths, and the shallower ones that keep arriving replace the deeper (filed first from the roots, a full
                    # bucket would hold only the shallowest positions there are and never be replaced)
                    eng.set_xcache(log2_entries)
                    prev = eng.xcache_stats()
                busy = (eng.status()[2].cpu().numpy() < PLAYOUTS) & ((eng.status()[0].cpu().numpy() & ~8) == 0)
                if mode == 1 and not busy.any():
                    break
                planes, need = eng.select(mode)
                need = need.cpu().numpy().astype(bool)
                lg = np.zeros((G, 2086), np.float32)
                v = np.zeros((G, 1), np.float32)
                if need.any():
                    lg[need], v[need] = fwd(planes[torch.from_numpy(need).to(planes.device)].cpu().numpy())
                eng.expand_backup(torch.from_numpy(lg).cuda(), torch.from_numpy(v).cuda())
                if ply == 0 and step < XC_FROM_STEP:
                    continue
                # the table after this launch: every entry one position's, no claim left open
                r = CC.check_xcache(eng.xcache_dump(), ref, mask=mask, max_ply=(ply + 1) * (PLAYOUTS + 2))
                dups = max(dups, r["duplicates"])
                st = eng.xcache_stats()
                filings.append(st["written"] + st["lost"] - prev["written"] - prev["lost"])
                prev = st
                launches += 1
            eng.set_sim_target(0)
            eng.set_terminal_extra(0)
            # the trees: the oracle's, all root statistics and whole trees of 256 of them
            hs = eng.root_stats_host()
            ost, ostatus, otrees = ostates[ply]
            for k in ("label", "N", "count"):
                assert np.array_equal(hs[k], ost[k][idx]), (ply, k)
            for k in ("Q", "P", "W"):
                assert np.array_equal(hs[k].view(np.uint32), ost[k][idx].view(np.uint32)), (ply, k)
            assert np.array_equal(eng.status()[0].cpu().numpy(), ostatus[idx]), ply
            for t in range(0, G, G // 256):
                assert np.array_equal(eng.tree_dump(t), otrees[idx[t]]), (ply, t)
            played = _played(hs)
            assert np.array_equal(played, _played(ost)[idx])
            eng.advance(played)
            # the per-tree entries after the re-root: every one still its node's (both compaction kernels, by parameter)
            rb, rs, _ = eng.root_state()
            rb, rs = rb.cpu().numpy(), rs.cpu().numpy()
            for t in list(range(0, G, G // 8)) + [G - 1]:
                ec_checked += CC.check_eval_cache(eng.eval_cache_dump(t), eng.tree_dump(t), rb[t], int(rs[t]), ref, mask=mask)
        st = eng.xcache_stats()
        print("cross-tree table of %d entries, %d-bit keys, advance kernel %s: %d launches checked, filings per launch median %d "
              "max %d, at most %d duplicate entries; %s; %d per-tree entries checked after re-roots" %
              (1 << log2_entries, key_bits, "global" if adv_global else "lds", launches, int(np.median(filings)), max(filings),
               dups, st, ec_checked))
        # not vacuous: the table is fought over in every launch, full buckets are replaced, swaps are lost, entries are lent
        assert st["replaced"] > 0 and st["lost"] > 0 and st["hits"] > 0
        assert np.median(filings) > 4 * 64 and max(filings) > 16 * 64
        assert ec_checked > 100
    finally:
        check(lib().cz_search_debug_advance_in_global_memory(h, 0), "cz_search_debug_advance_in_global_memory")
        eng.set_eval_cache(False)
        check(lib().cz_search_debug_eval_cache_key_bits(h, 64), "cz_search_debug_eval_cache_key_bits")


def _engine_expander(net, max_positions=256):
    """Reference priors and value for the real net: a SECOND engine, fresh trees rooted at the positions, one root expansion
    through the same step() path the self-play loop uses (net.search_eval + expand_backup_fc).  The priors are the roots'
    children's P; the root's value is not backed up anywhere (the root is never updated), so the value is taken from the
    value tensor that very expansion read (step's tap), negated as k_expand_backup files it."""
    from cchess_zero_amd.engine import SearchEngine
    eng2 = SearchEngine(max_positions, 4096, plane_dtype=torch.float16, channels=16)

    def expand(positions):
        out = []
        for a in range(0, len(positions), max_positions):
            chunk = positions[a:a + max_positions]
            k = len(chunk)
            eng2.reset(np.stack([p[0] for p in chunk]), np.array([p[1] for p in chunk], np.uint8), np.zeros(k, np.int32))
            seen = []
            eng2.step(net.forward_device, mode=0, tap=lambda planes, z, value: seen.append(value.float().cpu().numpy().copy()))
            assert len(seen) == 1 and not eng2.compact
            val = (seen[0].reshape(-1)[:k] * np.float32(-1.0)).astype(np.float32)
            st = eng2.root_stats_host()
            out += [(st["P"][i, :int(st["count"][i])].copy(), val[i]) for i in range(k)]
        return out
    return expand


def test_strict_selfplay_xcache_entries_match_a_fresh_expansion():
    """The product's self-play loop on the strict engine (precision "strict"), 1024 games from the start position, both cache
    levels on with a cross-tree table of 2^8 entries (four buckets, replaced all the time): after every ply every entry has the
    board, key, bucket, count, ordered labels and (src, dst) of its position exactly, and the priors and value a fresh root
    expansion of that position by a second engine with the same weights gives, bit for bit."""
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.net import PolicyValueNet
    from cchess_zero_amd.selfplay import SelfPlay
    from oracle import oracle as O
    Gs, playouts, plies = 1024, 32, 6
    net = PolicyValueNet(2, "cuda:0", torch.float16, seed=2, split="strict")
    eng = SearchEngine(Gs, 8192, plane_dtype=torch.float16, channels=16)
    sp = SelfPlay(eng, net, playouts, exploration=True, temperature=1.0, seed=5, eval_cache=True, xcache_log2=8)
    sp.start(np.tile(O.fen_to_board(O.START_FEN), (Gs, 1)), np.zeros(Gs, np.uint8), np.zeros(Gs, np.int32))
    eng.set_terminal_extra(4)
    assert net.fused_search and net.strict_report["engine"] == "mx6"
    ref = CC.Reference(_engine_expander(net))
    checked = 0
    try:
        for ply in range(plies):
            if ply == 2:
                # emptied two plies in: it then fills from retained subtrees (leaves of several depths), and the shallower leaves
                # that keep arriving must replace deeper entries — the replacement path is exercised whatever the first plies did
                eng.set_xcache(8)
            sp.run(1)
            r = CC.check_xcache(eng.xcache_dump(), ref, max_ply=(ply + 1) * (playouts + 2))
            checked += r["entries"]
        st = eng.xcache_stats()
        print("strict self-play, %d games x %d plies x %d playouts, cross-tree table of 256 entries: %d entries checked "
              "(%d distinct positions referenced); %s" % (Gs, plies, playouts, checked, len(ref.memo), st))
        assert checked >= plies * 200 and st["hits"] > 0 and st["replaced"] > 0 and st["lost"] > 0
        assert sp.stats()["stalled"] == 0
    finally:
        eng.set_terminal_extra(0)
        eng.set_eval_cache(False)
