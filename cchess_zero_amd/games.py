"""Recorded games -> training records: the bootstrap the reference does not have (it learns from its own self-play only,
cchess_main.selfplay, main.py:1493-1554).

  parse_games / write_games   games as MOVE LISTS in two text formats: one game per line of ICCS moves with an optional result
                              token ("h2e2 h9g7 ... 1-0"), and PGN-style blocks ([FEN "..."], [Result "..."], ICCS movetext
                              "1. H2-E2 H9-G7").  Anything that is not ICCS is reported and skipped, never guessed — unless
                              notations= names "wxf" and / or "chinese": such a game ("C2=5 H8+7", "炮二平五 馬8進7") is read to
                              TOKENS (notation.wxf_token / chinese_token) with no board, and the replay decodes them.
  GameReplayer.replay         cz_games_replay (csrc/cz_games.hip), or with a game of tokens cz_games_read (csrc/cz_notation.hip:
                              every token found among its position's legal moves inside the replay): all games in ONE launch,
                              one lane per game -> the packed
                              CZ_REC_* records selfplay.to_dense / records.RecordExpander take as they are (pi one-hot at the
                              played move, z the game's result from the mover's side), and for every game how far it is legal
                              under the rules asked for: "capture" (the reference's pseudo-legal moves) or "xiangqi" (king-safe).
  random_games                seeded playouts ply by ply out of the stand-alone Rules calls: the test corpus on the GPU and
                              the yardstick the fused replay is measured against (ply_by_ply_replay)
  pretrain                    supervised steps on such records with a holdout BY GAME, seeded and rank-consistent like
                              train.policy_update
  python -m cchess_zero_amd.games --in F [--rules xiangqi] [--notation any] [--out records.npy] [--write-pgn G.pgn [--write-notation wxf]]

Not read: binary formats (XQF, CBR); no repetition verdicts on imported games.
"""
import argparse
import collections
import json
import math
import random
import re
import sys

import numpy as np

from ._lib import (GAME_BLACK_KING_GONE, GAME_OK, GAME_RED_KING_GONE, GAME_STATUS, MAXMOVES, NSQ, POS_NO_SAFE_MOVE, REC_BYTES, REC_SIDE, REC_Z,
                   tables)
from .notation import NOTATIONS, START_FEN, chinese_token, fen_to_position, move_text, position_to_fen, wxf_token

# board: the 90 piece codes as bytes (comparable: parse_games(write_games(x)) == x); side 0 red / 1 black; rr: the restrict round
# of the start (a FEN's halfmove clock); labels: a tuple of move labels; result +1 red won / -1 black won / 0 draw / None
# unknown; tags: the other PGN tags as (name, value) pairs, in order; tokens: None, or — a game read from WXF / Chinese notation —
# a tuple of uint32 tokens (include/cchess_hip.h: cz_games_read), labels is then ()
Game = collections.namedtuple("Game", "board side rr labels result tags tokens", defaults=(None,))
_FORMAT_NAMES = {"ICCS": "iccs", "WXF": "wxf", "CHINESE": "chinese"}
_READERS = {"wxf": wxf_token, "chinese": chinese_token}
RESULT_TOKENS = {"1-0": 1, "0-1": -1, "1/2-1/2": 0, "*": None}
_TOKEN_OF = {1: "1-0", -1: "0-1", 0: "1/2-1/2", None: "*"}
_MOVE = re.compile(r"^([a-i][0-9])-?([a-i][0-9])$")
_TAG = re.compile(r'^\[\s*(\w+)\s+"(.*)"\s*\]$')
_DERIVED_TAGS = ("FEN", "Result", "Format")   # kept in Game.board / side / rr / result, written back from there


def _start():
    b, s, rr = fen_to_position(START_FEN)
    return bytes(b), s, rr


class GameList(list):
    """parse_games' answer: the games, and in .skipped what was left out as (first line, reason) pairs."""
    skipped = ()


def _iccs(t):
    m = _MOVE.match(t.lower())
    return m and tables()["label2i"].get(m.group(1) + m.group(2))


def _moves(tokens, where, notations=("iccs",), fmt=None):
    """movetext tokens -> (labels, tokens or None, result token or None).  The game's notation is fmt (its [Format] tag), or what
    its first move reads as among `notations`; every move is then read in that one notation, and ValueError names the text that
    is not a move in it."""
    return _moves_in(tokens, where, tuple(notations), fmt)


def _movetext(tokens):
    """the result tokens and the moves, without move numbers"""
    for t in tokens:
        if t in RESULT_TOKENS:
            yield t
            continue
        t = re.sub(r"^\d+\.+", "", t)   # "1." and "1..." glued to a move or alone
        if not t or set(t) == {"."}:
            continue
        yield t


def _reads(t, notation):
    if notation == "iccs":
        return _iccs(t) is not None
    try:
        _READERS[notation](t)
        return True
    except ValueError:
        return False


def _moves_in(tokens, where, notations, fmt):
    out, result, notation = [], None, fmt or ("iccs" if notations == ("iccs",) else None)
    for t in _movetext(tokens):
        if t in RESULT_TOKENS:
            result = t
            continue
        if notation is None:
            notation = next((n for n in NOTATIONS if n in notations and _reads(t, n)), None)
            if notation is None:
                raise ValueError("%s: %r is not a move in %s notation" % (where, t, " / ".join(n for n in NOTATIONS if n in notations)))
        if notation == "iccs":
            v = _iccs(t)
            if v is None:
                raise ValueError("%s: %r is not an ICCS move" % (where, t))
        else:
            try:
                v = _READERS[notation](t)
            except ValueError as e:
                raise ValueError("%s: %s" % (where, e))
        out.append(v)
    if notation in (None, "iccs"):
        return tuple(out), None, result
    return (), tuple(out), result


def parse_games(text, notations=("iccs",)):
    """Text -> GameList of Game.  With a line that starts with '[' the text is PGN-style blocks, else one game per line.
    notations: the move notations read, out of "iccs", "wxf", "chinese".  With more than ICCS named, a block's [Format] tag
    decides a game's notation, without a tag its first move does; a game in one notation never mixes another (it is skipped,
    the text named).  A WXF / Chinese game comes back with tokens instead of labels."""
    notations = tuple(notations)
    if not notations or any(n not in NOTATIONS for n in notations):
        raise ValueError("parse_games: notations are out of %r" % (NOTATIONS,))
    out, skipped = GameList(), []
    lines = text.splitlines()
    if not any(l.lstrip().startswith("[") for l in lines):
        for no, line in enumerate(lines, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            try:
                labels, toks, res = _moves(line.split(), "line %d" % no, notations)
            except ValueError as e:
                skipped.append((no, str(e)))
                continue
            b, s, rr = _start()
            out.append(Game(b, s, rr, labels, RESULT_TOKENS[res] if res else None, (), toks))
        out.skipped = tuple(skipped)
        return out
    # PGN-style: a block is its tag lines and the movetext behind them, up to the next tag line
    blocks, cur = [], None
    for no, line in enumerate(lines, 1):
        s = line.strip()
        if s.startswith("[") and (cur is None or cur["text"]):
            cur = dict(line=no, tags=[], text=[], bad=None)
            blocks.append(cur)
        if cur is None:
            if s:
                skipped.append((no, "line %d: text before the first tag" % no))
            continue
        if s.startswith("[") and not cur["text"]:
            m = _TAG.match(s)
            if m:
                cur["tags"].append((m.group(1), m.group(2)))
            else:
                cur["bad"] = "line %d: %r is not a tag" % (no, s)
        elif s:
            cur["text"].append(s)
    for blk in blocks:
        where = "block at line %d" % blk["line"]
        try:
            if blk["bad"]:
                raise ValueError(blk["bad"])
            tags = dict(blk["tags"])
            fmt = _FORMAT_NAMES.get(tags["Format"].strip().upper(), "") if "Format" in tags else None
            if fmt is not None and fmt not in notations:
                raise ValueError("%s: Format %r is not %s" % (where, tags["Format"], " / ".join(k for k, v in _FORMAT_NAMES.items() if v in notations)
                                                              if notations != ("iccs",) else "ICCS"))
            text = re.sub(r"\{[^}]*\}", " ", " ".join(blk["text"]))
            if "{" in text or "}" in text:
                raise ValueError("%s: unbalanced comment" % where)
            labels, toks, res = _moves(text.split(), where, notations, fmt)
            if "FEN" in tags:
                b, s, rr = fen_to_position(tags["FEN"])
                b = bytes(b)
            else:
                b, s, rr = _start()
            if "Result" in tags:
                if tags["Result"] not in RESULT_TOKENS:
                    raise ValueError("%s: Result %r" % (where, tags["Result"]))
                res = tags["Result"]
            out.append(Game(b, s, rr, labels, RESULT_TOKENS[res] if res else None, tuple(t for t in blk["tags"] if t[0] not in _DERIVED_TAGS), toks))
        except ValueError as e:
            skipped.append((blk["line"], str(e)))
    out.skipped = tuple(skipped)
    return out


def _plies(g):
    return g.labels if g.tokens is None else g.tokens


def _texts_from_replay(games, replay, notation):
    """per game the move texts in `notation` out of a replay's records (the board before every kept ply and the move played
    there), or None for a game whose plies are not all among the records, or with a ply the notation has no text for; and
    the games' decoded labels, or None likewise"""
    from ._lib import REC_LABELS, REC_VISITS
    rec = replay.records.cpu().numpy() if hasattr(replay.records, "cpu") else np.asarray(replay.records)
    lo = np.searchsorted(replay.game_of_record, np.arange(len(games)), "left")
    hi = np.searchsorted(replay.game_of_record, np.arange(len(games)), "right")
    texts, labels = [], []
    for g, game in enumerate(games):
        r = rec[lo[g]:hi[g]]
        if len(r) != len(_plies(game)):
            texts.append(None); labels.append(None)
            continue
        lab = np.ascontiguousarray(r[:, REC_LABELS:REC_LABELS + 2 * MAXMOVES]).view(np.uint16)
        vis = np.ascontiguousarray(r[:, REC_VISITS:REC_VISITS + 2 * MAXMOVES]).view(np.uint16)
        played = lab[np.arange(len(r)), vis.argmax(axis=1)] if len(r) else np.zeros(0, np.uint16)
        labels.append(tuple(int(x) for x in played))
        t = [move_text(r[i, :NSQ], int(r[i, REC_SIDE]), int(played[i]), notation) for i in range(len(r))]
        texts.append(None if any(x is None for x in t) else t)
    return texts, labels


def write_games(games, pgn=True, notation="iccs", replay=None):
    """The inverse of parse_games: parse_games(write_games(x)) == x.  pgn=False (one game per line) has no place for a start
    position or tags: ValueError for a game that has either.
    notation "wxf" / "chinese" (PGN form only) writes the moves in that notation under a [Format] tag.  That needs every ply's
    position: replay is GameReplayer.replay's answer for these very games, and a game is written from its records — the board
    before each ply and the move played there (notation.move_text).  A game with a ply that has no such text, or whose plies are
    not all among the records (it did not replay completely, or was dropped), is written whole as it came: ICCS from its labels,
    WXF from its tokens.  With a replay, a game of tokens that replayed completely can also be written as ICCS."""
    from .notation import token_text
    names = tables()["labels"]
    if notation not in NOTATIONS or (notation != "iccs" and (not pgn or replay is None)):
        raise ValueError("write_games: notation is one of %r; wxf and chinese need pgn=True and the games' replay" % (NOTATIONS,))
    games = list(games)
    texts, decoded = _texts_from_replay(games, replay, notation) if replay is not None else ([None] * len(games), [None] * len(games))
    out = []
    for gi, g in enumerate(games):
        fmt = "ICCS"
        if notation != "iccs" and texts[gi] is not None:
            mv, fmt = texts[gi], {"wxf": "WXF", "chinese": "Chinese"}[notation]
        elif g.tokens is None or decoded[gi] is not None:
            mv = [names[l] for l in (g.labels if g.tokens is None else decoded[gi])]
            mv = [m[:2].upper() + "-" + m[2:].upper() for m in mv] if pgn else mv
        else:
            mv, fmt = [token_text(t) for t in g.tokens], "WXF"
        if not pgn:
            if fmt != "ICCS":
                raise ValueError("write_games(pgn=False): a game of tokens needs the PGN form")
            if (g.board, g.side, g.rr) != _start() or g.tags:
                raise ValueError("write_games(pgn=False): a game with a start position or tags needs the PGN form")
            out.append(" ".join(mv + ([_TOKEN_OF[g.result]] if g.result is not None else [])))
            continue
        for k, v in g.tags:
            out.append('[%s "%s"]' % (k, v))
        if (g.board, g.side, g.rr) != _start():
            out.append('[FEN "%s"]' % position_to_fen(np.frombuffer(g.board, np.uint8), g.side, g.rr))
        out.append('[Format "%s"]' % fmt)
        out.append('[Result "%s"]' % _TOKEN_OF[g.result])
        out.append("")
        text = []
        if g.side and mv:
            text.append("1. ...")
        for i, m in enumerate(mv):
            k = i + (1 if g.side else 0)
            text.append(("%d. " % (k // 2 + 1) if k % 2 == 0 else "") + m)
        text.append(_TOKEN_OF[g.result])
        for i in range(0, len(text), 10):
            out.append(" ".join(text[i:i + 10]))
        out.append("")
    return "\n".join(out) + ("\n" if out else "")


def games_from_labels(moves, lens, results=None, boards=None, sides=None):
    """Arrays -> Games: moves [G, stride] labels, lens [G], results [G] (+1 / -1 / 0) or None, start boards [G, 90] / sides [G]
    or None (the opening position, red to move)."""
    b0, s0, rr0 = _start()
    return [Game(b0 if boards is None else bytes(np.asarray(boards[g], np.uint8)), s0 if sides is None else int(sides[g]), rr0,
                 tuple(int(x) for x in np.asarray(moves[g][:int(lens[g])]).astype(np.uint16)), None if results is None else int(results[g]), ())
            for g in range(len(lens))]


ReplayResult = collections.namedtuple("ReplayResult", "records game_of_record valid status end_flags final_boards final_side results kept counts labels")


def infer_result(end_flags, final_side):
    """The result the position a replay reached decides, or None: a missing king or a side to move without a king-safe move has
    lost."""
    if end_flags & GAME_RED_KING_GONE:
        return -1
    if end_flags & GAME_BLACK_KING_GONE:
        return 1
    if end_flags & POS_NO_SAFE_MOVE:
        return 1 if final_side else -1
    return None


class GameReplayer:
    """cz_games_replay / cz_games_read on a context of its own, or on a given one."""

    def __init__(self, ctx=None, device=0):
        from .engine import Context
        self.ctx = ctx or Context(1, 2, device)
        self.dev = self.ctx.device

    # From this many games on the upload is sorted by length.  A wave of 64 games runs as long as its longest game, so sorted
    # waves waste no lane-plies — which pays once the launch has more waves than the chip holds at a time (3 per CU, 256 CUs) and
    # the SUM of the waves' times decides.  Below that every wave has a SIMD to itself and the launch takes as long as its
    # longest wave, which sorting makes the heaviest (64 games that all go on to the last ply): 8192 games measured 4 % (capture)
    # and 13 % (xiangqi) slower sorted, 65 536 games 1.56x and 1.46x faster.
    SORT_FROM_GAMES = 64 * 3 * 256

    def replay(self, games, rules="capture", on_illegal="drop", sort=None):
        """games: Games -> ReplayResult.  The games are sorted by length (sort=None: from SORT_FROM_GAMES games on; True / False:
        always / never), uploaded once and replayed by one cz_games_replay call; rec_offset puts the records back in input order.
        records: a device tensor uint8 [n, 608] of the KEPT plies only, in input order; game_of_record int32 [n] (host): their
        games; valid, status, end_flags, final_boards, final_side (host, per game): the call's answers; results: per game +1 /
        -1 / 0, inferred from end_flags (infer_result) for a game that came without one, None where that says nothing; kept:
        which games' records are in `records`; counts: games per status name, and games, plies, kept_games, kept_plies,
        inferred_results, unknown_result, red_king_gone, black_king_gone, no_safe_move.
        on_illegal: "drop" keeps the games that replay completely, "truncate" also the legal part of the others.  A game whose
        result is unknown is dropped.  z is written by the kernel from the result given; for a game whose result is inferred
        the z bytes of its records are patched on the device afterwards (one masked write — no second replay).
        No game with tokens: cz_games_replay, as ever.  Otherwise cz_games_read for ALL of them in one launch, a game of labels
        passing its labels as small tokens; counts["ambiguous"] are the games a token stopped by naming two moves.  labels (the
        last field): uint16 [G, stride], the label every made ply was (decoded to), 0xFFFF elsewhere."""
        import torch
        from .rules import RULES
        if rules not in RULES or on_illegal not in ("drop", "truncate"):
            raise ValueError("GameReplayer.replay: rules is 'capture' or 'xiangqi', on_illegal 'drop' or 'truncate'")
        games = list(games)
        G = len(games)
        lens = np.array([len(_plies(g)) for g in games], np.int64)
        tokens = any(g.tokens is not None for g in games)
        if G == 0 or lens.max() > 65535 or lens.sum() >= 2 ** 31:
            if G:
                raise ValueError("GameReplayer.replay: a game longer than 65535 plies, or 2^31 plies in one call")
            return ReplayResult(torch.zeros((0, REC_BYTES), dtype=torch.uint8, device=self.dev), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros((0, NSQ), np.uint8), np.zeros(0, np.uint8), [], np.zeros(0, bool),
                                dict({k: 0 for k in GAME_STATUS}, games=0, plies=0, kept_games=0, kept_plies=0, inferred_results=0, unknown_result=0,
                                     red_king_gone=0, black_king_gone=0, no_safe_move=0), np.zeros((0, 1), np.uint16))
        stride, total = max(int(lens.max()), 1), int(lens.sum())
        order = np.argsort(lens, kind="stable") if (G >= self.SORT_FROM_GAMES if sort is None else sort) else np.arange(G)
        offset = np.concatenate([[0], np.cumsum(lens)[:-1]])
        moves = np.full((G, stride), 0xFFFF, np.uint32 if tokens else np.uint16)
        for j, g in enumerate(order):
            moves[j, :lens[g]] = _plies(games[g])
        start = _start()
        custom = any((g.board, g.side) != start[:2] for g in games)
        boards = np.stack([np.frombuffer(games[g].board, np.uint8) for g in order]) if custom else None
        side = np.array([games[g].side for g in order], np.uint8) if custom else None
        given = np.array([0 if games[g].result is None else games[g].result for g in order], np.int8)
        t = self.ctx.tensor
        d_moves, d_len, d_res, d_off = t(moves, torch.int32 if tokens else torch.int16), t(lens[order], torch.int32), t(given, torch.int8), t(offset[order], torch.int32)
        d_boards, d_side = t(boards, torch.uint8), t(side, torch.uint8)
        rec = torch.empty((total, REC_BYTES), dtype=torch.uint8, device=self.dev)
        valid = torch.empty(G, dtype=torch.int32, device=self.dev)
        status = torch.empty(G, dtype=torch.uint8, device=self.dev)
        flags = torch.empty(G, dtype=torch.uint8, device=self.dev)
        fboards = torch.empty((G, NSQ), dtype=torch.uint8, device=self.dev)
        fside = torch.empty(G, dtype=torch.uint8, device=self.dev)
        if tokens:
            d_labels = torch.empty((G, stride), dtype=torch.int16, device=self.dev)
            self.ctx.call("cz_games_read", d_boards, d_side, d_moves, stride, d_len, d_res, G, RULES[rules], d_off, total, rec, valid, status, flags,
                          fboards, fside, d_labels)
        else:
            self.ctx.call("cz_games_replay", d_boards, d_side, d_moves, stride, d_len, d_res, G, RULES[rules], d_off, total, rec, valid, status, flags,
                          fboards, fside)
        inv = np.empty(G, np.int64)
        inv[order] = np.arange(G)
        valid, status, flags = valid.cpu().numpy()[inv], status.cpu().numpy()[inv], flags.cpu().numpy()[inv]
        labels = d_labels.cpu().numpy().view(np.uint16)[inv] if tokens else np.where(np.arange(stride)[None, :] < valid[:, None], moves[inv], 0xFFFF).astype(np.uint16)
        fboards, fside = fboards.cpu().numpy()[inv], fside.cpu().numpy()[inv]
        results, inferred = [], np.zeros(G, bool)
        for g in range(G):
            r = games[g].result
            if r is None:
                r = infer_result(int(flags[g]), int(fside[g]))
                inferred[g] = r is not None
            results.append(r)
        known = np.array([r is not None for r in results])
        kept = known & ((status == GAME_OK) | (on_illegal == "truncate"))
        game_of = np.repeat(np.arange(G), lens)
        ply = np.arange(total) - offset[game_of]
        keep = kept[game_of] & (ply < valid[game_of])
        if inferred.any():   # z of the inferred results, on the device: the mover's view of the game's result
            res_of = torch.as_tensor(np.array([0 if r is None else r for r in results], np.int8)[game_of], device=self.dev)
            z = torch.where(rec[:, REC_SIDE] == 0, res_of, -res_of).view(torch.uint8)
            sel = torch.as_tensor(inferred[game_of] & keep, device=self.dev)
            rec[:, REC_Z] = torch.where(sel, z, rec[:, REC_Z])
        records = rec[torch.as_tensor(keep, device=self.dev)] if not keep.all() else rec
        counts = {name: int((status == i).sum()) for i, name in enumerate(GAME_STATUS)}
        counts.update(games=G, plies=total, kept_games=int(kept.sum()), kept_plies=int(keep.sum()), inferred_results=int((inferred & kept).sum()),
                      unknown_result=int((~known).sum()), red_king_gone=int((flags & GAME_RED_KING_GONE != 0).sum()),
                      black_king_gone=int((flags & GAME_BLACK_KING_GONE != 0).sum()), no_safe_move=int((flags & POS_NO_SAFE_MOVE != 0).sum()))
        return ReplayResult(records, game_of[keep].astype(np.int32), valid, status, flags, fboards, fside, results, kept, counts, labels)


def _playout(rules_obj, level, boards, side, max_ply, pick):
    """The ply-by-ply path of the stand-alone calls: per ply one move-list launch (movegen or movegen_kingsafe), pick(ply, moves,
    count) -> the labels to play (int16 [G]; -1 = none), one apply_move launch.  A game goes on while its label is in its list
    and both kings stand.  -> (played int16 [G, max_ply] (-1 behind a game's end), lens int32 [G], boards, side)."""
    import torch
    G = boards.shape[0]
    played = torch.full((G, max(max_ply, 1)), -1, dtype=torch.int16, device=boards.device)
    lens = torch.zeros(G, dtype=torch.int32, device=boards.device)
    alive = torch.ones(G, dtype=torch.bool, device=boards.device)
    for ply in range(max_ply):
        if level == "xiangqi":
            moves, count, _, _ = rules_obj.movegen_kingsafe(boards, side, want_mask=False)
        else:
            moves, count, _ = rules_obj.movegen(boards, side, want_mask=False)
        lab = pick(ply, moves, count)
        listed = ((moves == lab.unsqueeze(1)) & (torch.arange(MAXMOVES, device=boards.device).unsqueeze(0) < count.unsqueeze(1))).any(dim=1)
        go = alive & listed & (lab != -1)
        lab = torch.where(go, lab, torch.full_like(lab, -1))
        _, term = rules_obj.apply_move(boards, side, lab)       # label 0xFFFF leaves a game untouched
        played[:, ply] = lab
        lens += go.to(torch.int32)
        alive = go & (term == 0)
    return played, lens, boards, side


def random_games(rules, G, seed, max_ply, engine_rules=None, device=0):
    """G seeded uniform-random playouts from the opening position under the rule level `rules` ("capture": movegen, a game ends
    when a king is taken; "xiangqi": movegen_kingsafe, a game ends without a king-safe move), game g of U[0, max_ply] plies at the
    most, ply by ply out of the stand-alone Rules calls -> dict(moves uint16 [G, max_ply] (0xFFFF behind a game's end), lens int32
    [G], final_boards uint8 [G, 90], final_side uint8 [G]), host arrays."""
    import torch
    from .rules import RULES, START_BOARD, Rules
    if rules not in RULES:
        raise ValueError("random_games: rules is 'capture' or 'xiangqi'")
    R = engine_rules or Rules(device=device)
    gen = torch.Generator(device=R.dev).manual_seed(int(seed))
    boards = torch.from_numpy(np.tile(START_BOARD, (G, 1))).to(R.dev)
    side = torch.zeros(G, dtype=torch.uint8, device=R.dev)
    target = torch.randint(0, max_ply + 1, (G,), generator=gen, device=R.dev)

    def pick(ply, moves, count):
        cnt = count.to(torch.int64).clamp(min=0)
        r = (torch.rand(G, generator=gen, device=R.dev) * cnt.clamp(min=1)).to(torch.int64).clamp(max=MAXMOVES - 1)
        lab = moves.gather(1, r.unsqueeze(1)).squeeze(1)
        return torch.where((cnt > 0) & (target > ply), lab, torch.full_like(lab, -1))
    played, lens, boards, side = _playout(R, rules, boards, side, int(max_ply), pick)
    return dict(moves=played.cpu().numpy().view(np.uint16)[:, :max_ply], lens=lens.cpu().numpy(), final_boards=boards.cpu().numpy(),
                final_side=side.cpu().numpy())


def ply_by_ply_replay(rules, moves, lens, engine_rules=None, device=0):
    """The recorded moves through the same ply-by-ply path as random_games, its picks replaced by them: what a caller had to do
    before cz_games_replay, and the yardstick it is measured against (tools/rules_bench.py --replay).  moves: a DEVICE int16
    tensor [G, stride] or an array; lens [G] -> (valid int32 [G], final boards, final side), device tensors."""
    import torch
    from .rules import START_BOARD, Rules
    R = engine_rules or Rules(device=device)
    mv = R.ctx.tensor(moves, torch.int16)
    ln = R.ctx.tensor(lens, torch.int32)
    G, stride = mv.shape
    boards = torch.from_numpy(np.tile(START_BOARD, (G, 1))).to(R.dev)
    side = torch.zeros(G, dtype=torch.uint8, device=R.dev)
    none = torch.full((G,), -1, dtype=torch.int16, device=R.dev)
    valid, boards, side = _playout(R, rules, boards, side, stride, lambda ply, m, c: torch.where(ln > ply, mv[:, ply], none))[1:]
    return valid, boards, side


def holdout_split(game_of_record, holdout, seed):
    """-> (train record indices, holdout record indices, holdout games): the last ceil(holdout x games) games after a seeded
    shuffle of the sorted game numbers are held out, with all their records."""
    game_of_record = np.asarray(game_of_record)
    ids = sorted(set(int(g) for g in game_of_record))
    random.Random(int(seed)).shuffle(ids)
    n_hold = int(math.ceil(float(holdout) * len(ids))) if holdout > 0 else 0
    held = ids[len(ids) - n_hold:] if n_hold else []
    is_held = np.isin(game_of_record, np.array(held, game_of_record.dtype))
    return np.nonzero(~is_held)[0], np.nonzero(is_held)[0], held


def pretrain(net, records, game_of_record, steps, batch_size, learning_rate, seed, mirror=False, expand=None, holdout=0.05, log=print):
    """Supervised steps on replayed records.  net: train_step(planes, pi, z, lr) -> (accuracy, loss, global_step) and forward(planes)
    -> (logits, value), as train.policy_update's.  records: uint8 [n, 608], a host array or a device tensor; game_of_record [n].
    Holdout is by GAME (holdout_split).  Step s draws min(batch_size, training records) indices of the training part with
    random.Random((seed << 32) ^ s).sample, then — mirror=True — one coin per index from the same generator, as policy_update
    does; rank r of a process group trains on elements r::world of the draw (every rank draws the same) and train_step averages
    the gradients.  The mini-batch is built by expand (records.RecordExpander.expand: on the device) or by selfplay.to_dense of
    records.mirror_records.  At the end, on the held-out records and from net.forward: top1 (the net's best move is the played
    one), logloss (mean -log softmax(logits)[played]), value_sign (the share of records whose value has the sign of z).
    -> info dict(steps, losses, accuracies, train_records, holdout_records, holdout_games, mirrored, top1, logloss, value_sign)."""
    import torch
    import torch.distributed as dist
    from .records import mirror_records
    from .selfplay import to_dense
    on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    world, rank = (dist.get_world_size(), dist.get_rank()) if on else (1, 0)
    dev_rec = torch.is_tensor(records)
    train_idx, hold_idx, held = holdout_split(game_of_record, holdout, seed)
    if len(train_idx) == 0:
        raise ValueError("pretrain: no record is left to train on (%d records, %d held out)" % (len(game_of_record), len(hold_idx)))
    k = min(int(batch_size), len(train_idx))
    if k < world:
        raise ValueError("pretrain: %d samples per step for %d ranks: a rank would train on nothing" % (k, world))

    def take(idx):
        return records[torch.as_tensor(idx, device=records.device)] if dev_rec else np.asarray(records)[idx]

    def batch(idx, flags):
        rec = take(idx)
        if expand is not None:
            planes, pi, z = expand(rec, flags, 1.0)
            return planes, pi, z.reshape(-1, 1)
        rec = rec.cpu().numpy() if dev_rec else rec
        planes, pi, z = to_dense(mirror_records(rec, flags) if flags is not None else rec, 1.0, exact=True)
        return list(planes), list(pi), np.expand_dims(z, 1)

    losses, accs, mirrored = [], [], 0
    for s in range(int(steps)):
        rng = random.Random((int(seed) << 32) ^ s)
        draw = rng.sample(range(len(train_idx)), k)
        flags = np.array([rng.getrandbits(1) for _ in draw], np.uint8)[rank::world] if mirror else None
        idx = train_idx[np.array(draw)[rank::world]]
        acc, loss, _ = net.train_step(*batch(idx, flags), learning_rate)
        losses.append(float(loss)); accs.append(float(acc))
        mirrored += int(flags.sum()) if mirror else 0
        if s % 50 == 0 or s + 1 == steps:
            log("pretrain step {} loss {} accuracy {}".format(s, loss, acc))
    if on and hasattr(net, "module"):   # replicas stay bit-identical whatever the reduction order did, as after a policy update
        from .parallel import broadcast_weights
        broadcast_weights(net.module, src=0)
        if hasattr(net, "refresh"):
            net.refresh()
    info = dict(steps=int(steps), losses=losses, accuracies=accs, train_records=int(len(train_idx)), holdout_records=int(len(hold_idx)),
                holdout_games=len(held), mirrored=mirrored, top1=None, logloss=None, value_sign=None)
    if len(hold_idx):
        hit, ll, sign = 0, 0.0, 0
        for lo in range(0, len(hold_idx), max(int(batch_size), 1)):
            planes, pi, z = batch(hold_idx[lo:lo + max(int(batch_size), 1)], None)
            logits, v = net.forward(planes)
            logits, v = np.asarray(logits, np.float64), np.asarray(v, np.float64).reshape(-1)
            pi = pi.cpu().numpy() if torch.is_tensor(pi) else np.asarray(pi)
            z = (z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z)).reshape(-1)
            played = pi.argmax(axis=1)
            m = logits.max(axis=1, keepdims=True)
            logp = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
            hit += int((logits.argmax(axis=1) == played).sum())
            ll += float(-logp[np.arange(len(played)), played].sum())
            sign += int((np.sign(v) == np.sign(z)).sum())
        n = float(len(hold_idx))
        info.update(top1=hit / n, logloss=ll / n, value_sign=sign / n)
    return info


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.games", description="Recorded games (lines of moves or PGN-style blocks; ICCS, with --notation any also WXF and Chinese) -> packed training records")
    ap.add_argument("--in", dest="src", required=True, help="the games: one per line of ICCS moves, or PGN-style blocks with ICCS movetext")
    ap.add_argument("--rules", choices=("capture", "xiangqi"), default="capture")
    ap.add_argument("--on_illegal", choices=("drop", "truncate"), default="drop")
    ap.add_argument("--out", help="write the kept records here (numpy uint8 [n, 608]; <out>.games.npy: their games)")
    ap.add_argument("--write-pgn", dest="write_pgn", help="write the games read back as PGN-style blocks")
    ap.add_argument("--notation", choices=("iccs", "any"), default="iccs", help="the move notations read: ICCS only, or any of ICCS, WXF and Chinese")
    ap.add_argument("--write-notation", dest="write_notation", choices=NOTATIONS, default="iccs", help="the notation --write-pgn writes (from the replay)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    games = parse_games(open(a.src, encoding="utf-8").read(), notations=NOTATIONS if a.notation == "any" else ("iccs",))
    plain = a.write_notation == "iccs" and not any(g.tokens is not None for g in games)
    if a.write_pgn and plain:
        open(a.write_pgn, "w").write(write_games(games, pgn=True))
    r = GameReplayer(device=a.device).replay(games, rules=a.rules, on_illegal=a.on_illegal)
    if a.write_pgn and not plain:   # the positions come from the replay
        open(a.write_pgn, "w", encoding="utf-8").write(write_games(games, pgn=True, notation=a.write_notation, replay=r))
    if a.out:
        np.save(a.out, r.records.cpu().numpy())
        np.save(a.out + ".games.npy", r.game_of_record)
    c = r.counts
    print(json.dumps(dict(games=c["games"], plies=c["plies"], kept_games=c["kept_games"], kept_plies=c["kept_plies"], rules=a.rules,
                          status={k: c[k] for k in GAME_STATUS}, endings=dict(red_king_gone=c["red_king_gone"], black_king_gone=c["black_king_gone"],
                                                                              no_safe_move=c["no_safe_move"]),
                          inferred_results=c["inferred_results"], unknown_result=c["unknown_result"], skipped_blocks=[list(s) for s in games.skipped])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
