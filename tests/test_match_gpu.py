"""Evaluation matches on the GPU (cchess_zero_amd/arena.py over csrc/cz_match.hip): every game of a fakenet match equals
the CPU oracle's replay (tests/match_model.py), a net against itself is colour-symmetric, the kernels' edge cases follow the
model, random openings are distinct and legal, the facade's policy_evaluate / --eval_every, two ranks on one device."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_model as MM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_players(pa=24, pb=16):
    return [(MM.device_forward("pos", 11), pa), (MM.device_forward("signed", 12), pb)]


def _host_players(pa=24, pb=16):
    import fakenet
    return [(fakenet.make_forward("pos", 11), pa), (fakenet.make_forward("signed", 12), pb)]


@pytest.fixture(scope="module")
def openings8():
    from cchess_zero_amd.arena import random_openings
    return random_openings(8, 4, seed=11)


# ---- 1. oracle replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_plies", [0, 6])
def test_match_equals_oracle_replay(openings8, sample_plies):
    from cchess_zero_amd.arena import Match
    want = MM.play_match(_host_players(), openings8, max_plies=160, sample_plies=sample_plies, seed=5)
    for slots in (16, 6):   # 6 slots: the queue re-seeds slots as games end
        m = Match(*_fake_players(), openings8, slots=slots, max_plies=160, sample_plies=sample_plies, seed=5, nodes_per_tree=1 << 15)
        res = m.play()
        MM.assert_equals_model(res, want, slots)
        assert res.simulations > 0 and res.sims_per_s > 0


# ---- 2. a real net against itself ----------------------------------------------------------------------------------------
def test_self_match_with_a_real_net_is_colour_symmetric(openings8):
    from cchess_zero_amd.arena import Match
    from cchess_zero_amd.net import PolicyValueNet
    net = PolicyValueNet(2, "cuda:0", torch.float16, seed=3, split="strict")
    res = Match((net, 32), (net, 32), openings8, slots=16, max_plies=200).play()
    for p in range(8):
        a, b = 2 * p, 2 * p + 1
        assert res.moves[a] == res.moves[b], p            # the same net with the same budget plays red in both games
        assert res.a_red[a] == 1 and res.a_red[b] == 0
        assert res.result[a] == -res.result[b] and res.reason[a] == res.reason[b]
    assert res.aborted == 0 and res.score == 0.5


# ---- 3. kernel edges against the model -----------------------------------------------------------------------------------
def _const_forward(value=0.0, prefer=()):
    """logits 1 on the `prefer` labels (both orientations), 0 elsewhere — all 1 without a preference; constant value."""
    from cchess_zero_amd._lib import tables
    unflip = tables()["unflip"]
    idx = sorted(set(int(x) for x in prefer) | set(int(unflip[int(x)]) for x in prefer))

    def forward(planes):
        B = planes.shape[0]
        lg = torch.zeros((B, 2086), dtype=torch.float32, device=planes.device) if idx else torch.ones((B, 2086), dtype=torch.float32, device=planes.device)
        if idx:
            lg[:, idx] = 1.0
        return lg, torch.full((B, 1), float(value), dtype=torch.float32, device=planes.device)
    return forward


def _one_opening(board, side=0, rr=0):
    from cchess_zero_amd.arena import Openings
    return Openings(np.asarray(board, np.uint8)[None], [side], [rr])


def _start():
    from oracle import oracle as O
    return O.fen_to_board(O.START_FEN)


def test_greedy_tie_takes_the_first_maximum():
    from cchess_zero_amd.arena import Match
    ties = 0
    for v in (0.5, -0.5):
        f = (_const_forward(v), 5)
        m = Match(f, f, _one_opening(_start()), slots=2, max_plies=4)
        m.start()
        m.search(0)
        m.search(1)
        N = [m.engines[p].root_stats_host() for p in (0, 1)]
        m.choose()
        played = m.played.cpu().numpy().view(np.uint16)
        for g, mover in ((0, 0), (1, 1)):   # game 0: A red moves, game 1: B red moves
            n = int(N[mover]["count"][g])
            vis = N[mover]["N"][g, :n]
            assert played[g] == N[mover]["label"][g, MM.choose(vis, 9, 0, 0, g)]
            ties += int((vis == vis.max()).sum() > 1)
        m.close()
    assert ties >= 1   # one of the two value signs spreads the visits over several children: a tie at the maximum


def _king_board():
    """Red king e0, black king d9, red rook d5 (takes the black king up the d file), black rook e5 (takes the red king)."""
    b = np.zeros(90, np.uint8)
    b[4], b[84], b[48], b[49] = 1, 8, 3, 10
    return b


@pytest.mark.parametrize("side", [0, 1])
def test_king_captured_by_red_and_by_black(side):
    from oracle import oracle as O
    from cchess_zero_amd.arena import Match
    b = _king_board()
    mv = O.legal_moves(b, side)
    cap = [int(l) for l in mv if O.apply_move(b, int(l))[1] in (1, 8)]
    assert len(cap) == 1
    # at the root U = 0 (its N is never updated, quirk Q2) and a net value of +0.5 backs up Q = -0.5: the playouts visit the
    # children in generation order until the capture, whose Q = +1 then takes every further playout
    f = (_const_forward(0.5), len(mv) + 4)
    res = Match(f, f, _one_opening(b, side), slots=2, max_plies=8).play()
    assert res.reason.tolist() == [MM.KING, MM.KING] and res.plies.tolist() == [1, 1]
    after = O.apply_move(b, cap[0])[0]
    # the mover wins: game 0 has A red, game 1 B red
    want = [MM.adjudicate(after, 0, 1, 8, False, g == 0)[1] for g in (0, 1)]
    assert res.result.tolist() == want == ([1, -1] if side == 0 else [-1, 1])
    assert res.moves[0] == res.moves[1] and len(res.moves[0]) == 1


def test_restrict_round_59_to_60_is_a_draw_and_the_ply_cap_too():
    from cchess_zero_amd.arena import Match
    f = (_const_forward(0.0), 2)
    res = Match(f, f, _one_opening(_start(), 0, 59), slots=2, max_plies=8).play()
    assert res.reason.tolist() == [MM.RR60, MM.RR60] and res.plies.tolist() == [1, 1] and res.result.tolist() == [0, 0]
    res = Match(*_fake_players(4, 3), _one_opening(_start()), slots=2, max_plies=3).play()
    assert res.reason.tolist() == [MM.PLY_CAP, MM.PLY_CAP] and res.plies.tolist() == [3, 3] and res.result.tolist() == [0, 0]
    assert res.score == 0.5 and res.draws == 2


def test_mover_without_a_child_aborts():
    from cchess_zero_amd.arena import Match
    # 16 nodes per tree: the start position's 44 children do not fit, the root stays unexpanded
    res = Match(*_fake_players(4, 3), _one_opening(_start()), slots=2, max_plies=8, nodes_per_tree=16).play()
    assert res.reason.tolist() == [MM.ABORTED, MM.ABORTED] and res.plies.tolist() == [0, 0]
    assert res.aborted == 2 and res.scored == 0 and res.score is None


def _subtree(dump, label):
    """Records below the depth-0 child `label` of a tree_dump, one level up."""
    i = int(np.nonzero((dump[:, 0] == 0) & (dump[:, 1] == label))[0][0])
    j = i + 1
    while j < len(dump) and dump[j, 0] > 0:
        j += 1
    out = dump[i + 1:j].copy()
    out[:, 0] -= 1
    return out


def test_follower_keeps_its_subtree_or_starts_a_fresh_root_and_parked_slots_stay_idle():
    from cchess_zero_amd.arena import Match
    m = Match(*_fake_players(24, 16), _one_opening(_start()), slots=2, max_plies=3)
    m.start()
    # ply 0: game 0 (slot 0) A moves, game 1 (slot 1) B moves; the followers' roots were never expanded
    m.search(0)
    m.search(1)
    m.choose()
    m.follow()
    m.adjudicate()
    st = [m.engines[p].status() for p in (0, 1)]
    assert int(st[1][0][0]) == 0 and int(st[0][0][1]) == 0            # follower: status 0 (no BAD_ADVANCE left)
    assert len(m.engines[1].tree_dump(0)) == 0 and len(m.engines[0].tree_dump(1)) == 0   # a fresh, unexpanded root
    assert m.active()[0].tolist() == [0, 1] and m.active()[1].tolist() == [1, 0]
    # ply 1: the former movers follow the reply; their tree below it is kept as it was
    m.search(0)
    m.search(1)
    m.choose()
    played = m.played.cpu().numpy().view(np.uint16).copy()
    before = [m.engines[0].tree_dump(0), m.engines[1].tree_dump(1)]
    m.follow()
    m.adjudicate()
    after = [m.engines[0].tree_dump(0), m.engines[1].tree_dump(1)]
    for k in range(2):
        assert np.array_equal(after[k], _subtree(before[k], int(played[k])))
    assert int(m.engines[0].status()[0][0]) == 0 and int(m.engines[1].status()[0][1]) == 0
    # ply 2 ends both games at the ply cap; the queue is empty: both slots park
    m.step_ply()
    assert m.finished()[0] == 2
    a, b, game = m.active()
    assert not a.any() and not b.any() and game.tolist() == [-1, -1]
    m.search(0)
    m.search(1)
    for p in (0, 1):
        assert m.engines[p].status()[2].cpu().numpy().tolist() == [0, 0]
    assert m.results()["reason"].tolist() == [MM.PLY_CAP, MM.PLY_CAP]
    m.close()


# ---- 4. openings ---------------------------------------------------------------------------------------------------------
def test_random_openings_are_distinct_legal_and_reproducible():
    from oracle import oracle as O
    from cchess_zero_amd.arena import random_openings
    op = random_openings(512, 4, seed=7)
    assert len(op) == 512 and len(set(op.keys.tolist())) == 512
    assert ((op.boards == 1).any(axis=1) & (op.boards == 8).any(axis=1)).all()
    for i in range(512):
        b, s = _start(), 0
        for lab in op.moves[i]:
            assert lab in O.legal_moves(b, s).tolist(), (i, lab)
            b = O.apply_move(b, lab)[0]
            s ^= 1
        assert np.array_equal(b, op.boards[i]) and s == op.side[i] and O.zhash(b, s) == int(op.keys[i])
    again = random_openings(512, 4, seed=7)
    assert np.array_equal(again.keys, op.keys) and np.array_equal(again.boards, op.boards)


# ---- 5. facade -----------------------------------------------------------------------------------------------------------
def test_policy_evaluate_reports_the_score_and_changes_no_weight(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    from main import cchess_main
    cm = cchess_main(playout=16, res_block_nums=2, games=32)
    before = {k: v.detach().clone() for k, v in cm.policy_value_netowrk.module.state_dict().items()}
    step = cm.global_step
    w = cm.policy_evaluate(15)   # rounded up to 16 games
    r = cm.last_evaluation
    assert r.games == 16 and r.scored > 0 and w == pytest.approx((r.wins + 0.5 * r.draws) / r.scored)
    after = cm.policy_value_netowrk.module.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before) and cm.global_step == step
    cm.log_file.close()


def _main_train(tmp_path, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--mode", "train", "--games", "64", "--train_playout", "8", "--max_batches", "1",
           "--res_block_nums", "2"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    log = open(os.path.join(str(tmp_path), "log_file.txt")).read()
    return [l for l in p.stdout.splitlines() if l.startswith("evaluation:")], [l for l in log.splitlines() if l.startswith("evaluation:")]


def test_eval_every_writes_one_evaluation_line(tmp_path):
    import json
    out, log = _main_train(tmp_path, ["--eval_every", "1", "--eval_games", "16"])
    assert len(out) == 1 and out == log
    d = json.loads(out[0][len("evaluation:"):])
    assert d["games"] == 16 and d["batch"] == 1
    (tmp_path / "off").mkdir()
    out, log = _main_train(tmp_path / "off", [])
    assert out == [] and log == []


# ---- 6. two ranks on one device ------------------------------------------------------------------------------------------
def _rank(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    torch.cuda.set_device(0)   # both ranks on device 0 (CCHESS_ALL_ON_DEVICE0), gloo between them
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cchess_zero_amd.arena import Match, random_openings
    res = Match(*_fake_players(12, 8), random_openings(5, 4, seed=2), slots=4, max_plies=60, sample_plies=2, seed=3).play()
    q.put((rank, res.result.tolist(), res.plies.tolist(), res.reason.tolist(), res.moves, res.simulations))
    dist.monitored_barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_device_return_the_world1_result():
    import torch.multiprocessing as mp
    from cchess_zero_amd.arena import Match, random_openings
    one = Match(*_fake_players(12, 8), random_openings(5, 4, seed=2), slots=4, max_plies=60, sample_plies=2, seed=3).play()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in got:
        assert r[1] == one.result.tolist() and r[2] == one.plies.tolist() and r[3] == one.reason.tolist() and r[4] == one.moves
        assert r[5] == one.simulations
