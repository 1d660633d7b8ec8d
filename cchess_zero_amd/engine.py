"""Lock-step search engine over G game trees (host side of K1-K7).

PyTorch is used only for device memory / streams; every search operation is one HIP kernel
launched through the C-ABI (include/cchess_hip.h).  Mirrors, for G trees at once, what the
reference's MCTS_tree (main.py:234-577) does for one.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F16, F32, MAXMOVES, NLABELS, NSQ, _ptr, call, lib, out_pointers   # noqa: F401 (_ptr: tests and tools import it from here)


# The evaluation cache's dump formats (include/cchess_hip.h; csrc/cz_evalcache.h states the same field list for the kernels).
# Cross-tree table of n entries: field after field, (name, element type, elements per entry, bytes per entry of the fields
# before it), with XC_COUNTER_BYTES between the keys and the rest — per entry 8 + 4 + 4 + 48 + 256 + 256 + 512 = 1088 bytes.
XC_FIELDS, XC_ENTRY_BYTES, XC_COUNTER_BYTES = [], 0, 64
for _name, _dt, _per in (("key", np.uint64, 1), ("value", np.float32, 1), ("count_ply", np.uint32, 1), ("board", np.uint32, 12),
                         ("label", np.uint16, MAXMOVES), ("sd", np.uint16, MAXMOVES), ("P", np.float32, MAXMOVES)):
    XC_FIELDS.append((_name, _dt, _per, XC_ENTRY_BYTES))
    XC_ENTRY_BYTES += np.dtype(_dt).itemsize * _per
EC_ENTRIES = 128 * 64   # per-tree level: 128 buckets x 64 entries per tree


def plane_format(forward):
    """(plane dtype, channels) the select kernel writes a player's leaf planes in: a PolicyValueNet on the fused path (hip
    backend, or the strict ladder) reads 16 channels of its 16-bit type straight from the select kernel; any other net or a
    plain forward(planes) -> (logits, value) callable gets the reference's 14 float32 planes."""
    net = getattr(forward, "__self__", forward)
    dtype = getattr(net, "dtype", None)
    fused = hasattr(net, "strict_auto") and (net.backend == "hip" or net.strict_auto) and dtype in (torch.float16, torch.bfloat16)
    return (dtype, 16) if fused else (torch.float32, 14)


def pool_nodes(playouts):
    """Node pool per tree for a search of `playouts` simulations per move: a ply adds ~40 nodes per simulation on top of the
    subtree kept from the previous ply; a tree that fills its pool stops expanding for the rest of that ply (the move is
    chosen from the visits it has) and gets its room back when cz_search_advance compacts it."""
    return max(4096, (int(playouts) + 2) * 128)


class Context:
    """Owns a cz_ctx bound to one GPU and to torch's current stream on it."""

    def __init__(self, max_games, max_nodes_per_tree, device=0):
        if not torch.cuda.is_available():
            raise _lib.CchessHipError("no HIP device visible: the cchess_hip path needs an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", device)
        self.max_games = int(max_games)
        self.cap = int(max_nodes_per_tree)
        h = C.c_void_p()
        call("cz_create", device, self.max_games, self.cap, C.byref(h))
        self.h = h
        self.bind_stream()

    def bind_stream(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        call("cz_set_stream", self.h, s.cuda_stream)

    def call(self, name, *args):
        """_lib.call(name, <this context>, *args) on torch's CURRENT stream (also under HIP graph capture): every launch binds."""
        self.bind_stream()
        return call(name, self.h, *args)

    def tensor(self, x, dtype):
        """tensor / array / None -> contiguous `dtype` tensor on the context's device (None stays None).  torch has no wide
        unsigned types: a u16 / u32 / u64 array (labels, keys) goes as its bits."""
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(x)
            if x.dtype.kind == "u" and x.dtype.itemsize > 1:
                x = x.view("i%d" % x.dtype.itemsize)
            x = torch.as_tensor(x)
        return x.to(self.device).to(dtype).contiguous()

    def mask(self, active):
        """An active-mask argument: a raw device pointer (cz_selfplay_active, cz_match_active) as it is, else tensor(.., uint8)."""
        return active if isinstance(active, C.c_void_p) else self.tensor(active, torch.uint8)

    def download(self, ptr, dtype, shape):
        """cz_download of the device pointer `ptr` -> a new numpy array (synchronises)."""
        out = np.empty(shape, dtype)
        self.call("cz_download", out.ctypes.data, ptr, out.nbytes)
        return out

    def synchronize(self):
        call("cz_synchronize", self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().cz_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SearchEngine:
    """G trees searched in lock-step: select -> (batched net) -> expand_backup."""

    def __init__(self, max_games, max_nodes_per_tree, device=0, plane_dtype=torch.float32, channels=14, ctx=None, width=1):
        """width = simulations in flight per tree and step (the reference's search_threads); 1 = sequential."""
        self.ctx = ctx or Context(max_games, max_nodes_per_tree, device)
        self.width = int(width)
        if self.width > 1:
            self.ctx.call("cz_search_set_width", self.width)
        self.dev = self.ctx.device
        self.G = 0
        self.channels = int(channels)
        self.plane_dtype = plane_dtype
        self._pd = {torch.bfloat16: BF16, torch.float16: F16}.get(plane_dtype, F32)
        # step(): compact evaluation batches on the fused-net path.  Off by default: at 8192 trees the trunk needs
        # ceil(rows / 1024) workgroup rounds, so dropping the ~9 % terminal leaves of the bench workload removes no round
        # (and the row counter costs 60 us of atomics); self-play switches it on, where finished games park their trees.
        self.compact = False
        self.planes = None
        self.need = None
        self.terminal_extra = 0
        self.eval_cache = False
        self.xcache_log2 = 0

    def set_terminal_extra(self, n):
        """Terminal simulations (king captured / 60-ply rule: no net evaluation needed, main.py:409-416) a tree may complete
        inside one select launch before it presents a leaf that does need the net (cz_search_set_terminal_extra).  Trees
        stay bit-identical; a lock-step then completes more than one simulation per net row.  Width 1 only."""
        assert self.width == 1 or int(n) == 0, "terminal_extra applies to the one-simulation-per-tree select"
        self.ctx.call("cz_search_set_terminal_extra", int(n))
        self.terminal_extra = int(n)

    def set_eval_cache(self, on):
        """Evaluation cache (include/cchess_hip.h: cz_search_set_eval_cache): a leaf whose position the tree has
        evaluated before is expanded from the remembered node inside the select launch, without a net row.  A hit is
        taken only when the stored position equals the leaf's (a key collision is a miss); up to 4 hits per tree and
        launch, independently of set_terminal_extra."""
        assert self.width == 1 or not on, "the evaluation cache needs one simulation in flight per tree"
        self.ctx.call("cz_search_set_eval_cache", 1 if on else 0)
        self.eval_cache = bool(on)
        if not on:
            self.xcache_log2 = 0    # the cross-tree level lives behind the per-tree probe: the library frees it with it

    def set_xcache(self, log2_entries):
        """Cross-tree level of the evaluation cache (cz_search_set_xcache; needs set_eval_cache(True)): one table of
        2**log2_entries self-contained entries (1088 bytes each) shared by all trees of the context — a leaf whose position ANY
        tree has evaluated is expanded inside the select launch from the remembered row (verified against the stored position;
        trees bit-identical).  0 frees it; calling it again empties it (do so whenever the weights change — set_eval_cache(True)
        empties both levels)."""
        assert self.eval_cache or not log2_entries, "set_eval_cache(True) first"
        self.ctx.call("cz_search_set_xcache", int(log2_entries))
        self.xcache_log2 = int(log2_entries)

    def xcache_stats(self):
        """-> dict(hits, lookups, written, lost, replaced) of the cross-tree level since it was last emptied: lost = filings that
        found no room (a full bucket of shallower positions, or every swap lost), replaced = entries that took a deeper one's
        place (part of `written`)."""
        a = (C.c_ulonglong * 5)()
        self.ctx.call("cz_search_xcache_stats5", a)
        return dict(hits=int(a[0]), lookups=int(a[1]), written=int(a[2]), lost=int(a[3]), replaced=int(a[4]))

    def xcache_dump(self):
        """(tests) The cross-tree table as it stands (cz_search_debug_xcache_dump): dict of numpy arrays over its n entries —
        key u64 [n] (0 = empty), value f32 [n], count u16 [n], ply u16 [n], board u32 [n, 12] (the packed position),
        label u16 [n, 128], sd u16 [n, 128] (src | dst << 8), P f32 [n, 128].  The raw block is n * 1088 + 64 bytes, laid out by
        XC_FIELDS; count and ply are the low and high half of its count word."""
        n = self.ctx.call("cz_search_debug_xcache_dump", None, 0)
        raw = np.zeros(n * XC_ENTRY_BYTES + XC_COUNTER_BYTES, np.uint8)
        self.ctx.call("cz_search_debug_xcache_dump", raw.ctypes.data, raw.nbytes)
        out = {}
        for name, dt, per, before in XC_FIELDS:
            off = n * before + (XC_COUNTER_BYTES if before else 0)   # the counter block sits behind the keys
            out[name] = raw[off:off + n * per * np.dtype(dt).itemsize].view(dt).reshape((n, per) if per > 1 else (n,)).copy()
        cnt = out.pop("count_ply")
        out.update(count=(cnt & 0xFFFF).astype(np.uint16), ply=(cnt >> 16).astype(np.uint16))
        return out

    def eval_cache_dump(self, g):
        """(tests) Tree g's per-tree cache entries (cz_search_debug_eval_cache_dump): dict of numpy arrays over its 8192 entries —
        key u64 (0 = empty), node i32, value f32, board u32 [8192, 12], record i32 (the node's row in tree_dump(g), -1 = the root,
        -2 = not in the tree)."""
        n = EC_ENTRIES
        out = dict(key=np.zeros(n, np.uint64), node=np.zeros(n, np.int32), value=np.zeros(n, np.float32),
                   board=np.zeros((n, 12), np.uint32), record=np.zeros(n, np.int32))
        p = [out[k].ctypes.data for k in ("key", "node", "value", "board", "record")]
        assert self.ctx.call("cz_search_debug_eval_cache_dump", int(g), *p) == n
        return out

    def eval_cache_stats(self):
        """-> (hits, lookups) summed over the trees since the cache was turned on."""
        h, n = C.c_ulonglong(0), C.c_ulonglong(0)
        self.ctx.call("cz_search_eval_cache_stats", C.byref(h), C.byref(n))
        return int(h.value), int(n.value)

    def eval_cache_collisions(self):
        """Key matches the cache refused because the stored position differed from the leaf's (taken as misses)."""
        n = C.c_ulonglong(0)
        self.ctx.call("cz_search_eval_cache_collisions", C.byref(n))
        return int(n.value)

    def set_sim_target(self, target):
        """Trees stop at `target` completed simulations since their last reset / advance (0: no limit)."""
        self.ctx.call("cz_search_set_sim_target", int(target))

    # -- tree lifecycle ------------------------------------------------------------------------
    def reset(self, boards, side, rr=None):
        t = self.ctx.tensor
        boards, side, rr_t = t(boards, torch.uint8).reshape(-1, NSQ), t(side, torch.uint8), t(rr, torch.int32)
        G = boards.shape[0]
        self.ctx.call("cz_search_reset", boards, side, rr_t, G)
        if self.G != G or self.planes is None:
            self.G = G
            self.planes = torch.zeros((G * self.width, 9, 10, self.channels), dtype=self.plane_dtype, device=self.dev)
            self.need = torch.zeros(G * self.width, dtype=torch.uint8, device=self.dev)
        self._keep = (boards, side, rr_t)

    def reload(self, which, boards, side, rr=None):
        """MCTS_tree.reload / GameBoard.reload for the games that are over (main.py:255-258,604-608): trees with
        which[g] != 0 start afresh from boards[g] / side[g] / rr[g] ([G] arrays), the others are untouched."""
        t = self.ctx.tensor
        which, boards, side = t(which, torch.uint8), t(boards, torch.uint8).reshape(-1, NSQ), t(side, torch.uint8)
        assert which.numel() == self.G and boards.shape[0] == self.G and side.numel() == self.G
        self.ctx.call("cz_search_reload", which, boards, side, t(rr, torch.int32))

    def select(self, mode=1, active=None, k=None):
        """-> (leaf planes [G*k,9,10,C] device tensor, needs_eval [G*k] u8 device tensor); k <= width descents per
        tree (default: the engine's width)."""
        k = self.width if k is None else int(k)
        self._k = k
        self._act = act = self.ctx.mask(active)
        if self.width > 1:
            self.ctx.call("cz_search_select_k", int(mode), k, act, self.planes, self._pd, self.channels, self.need)
            return self.planes[:self.G * k], self.need[:self.G * k]
        self.ctx.call("cz_search_select", int(mode), act, self.planes, self._pd, self.channels, self.need)
        return self.planes, self.need

    def expand_backup(self, logits, value):
        """logits [G,2086], value [G,1] or [G]: float32 or bfloat16 device tensors."""
        if logits.dtype != value.dtype:
            value = value.to(logits.dtype)
        dt = BF16 if logits.dtype == torch.bfloat16 else F32
        if dt == F32 and logits.dtype != torch.float32:
            logits, value = logits.float(), value.float()
        logits = logits.contiguous()
        value = value.contiguous()
        k = getattr(self, "_k", self.width)
        assert logits.shape == (self.G * k, NLABELS) and value.numel() == self.G * k
        if self.width > 1:
            self.ctx.call("cz_search_expand_backup_k", k, logits, value, dt)
        else:
            self.ctx.call("cz_search_expand_backup", logits, value, dt)

    def expand_backup_fc(self, z, value, pfc_w, pfc_b, compact=False):
        """expand_backup with the policy FC folded in (cz_search_expand_backup_fc): z [G,90,3] f32 head-conv outputs,
        value [G] or [G,1] f32, pfc_w [2086,180] f32 (torch layout), pfc_b [2086] f32.  Width 1 only.
        compact=True: z / value rows are the ones select_compact handed out (tree g -> row slot_of[g])."""
        assert self.width == 1, "expand_backup_fc pairs with the one-simulation-per-tree select"
        assert z.dtype == torch.float32 and z.is_contiguous() and z.shape == (self.G, 90, 3)
        value = value.float().contiguous()
        assert value.numel() == self.G and pfc_w.is_contiguous() and pfc_w.shape == (NLABELS, 180) and pfc_b.numel() == NLABELS
        self.ctx.call("cz_search_expand_backup_fc", z, value, pfc_w, pfc_b, 1 if compact else 0)

    def select_compact(self, mode=1, active=None):
        """select() with compact evaluation batches: the leaf planes of the trees that need a net evaluation go to rows
        0 .. n-1 of the planes buffer (cz_search_select_compact).  Returns (planes, n_rows_ptr): the full planes tensor and
        the DEVICE address of n (an int), to be handed to the net through set_batch_count — no host synchronisation."""
        assert self.width == 1
        self._act = act = self.ctx.mask(active)
        self.ctx.bind_stream()   # the one launch that is also a getter: not through ctx.call
        _, n_p = out_pointers("cz_search_select_compact", self.ctx.h, 2, int(mode), act, self.planes, self._pd, self.channels)
        return self.planes, n_p

    def eval_totals(self):
        """(rows evaluated, compact steps) since the context was created (synchronises)."""
        r, n = C.c_ulonglong(0), C.c_ulonglong(0)
        self.ctx.call("cz_search_eval_totals", C.byref(r), C.byref(n))
        return int(r.value), int(n.value)

    def root_stats(self):
        G, dev = self.G, self.dev
        out = dict(label=torch.empty((G, MAXMOVES), dtype=torch.int16, device=dev),
                   N=torch.empty((G, MAXMOVES), dtype=torch.int32, device=dev),
                   Q=torch.empty((G, MAXMOVES), dtype=torch.float32, device=dev),
                   P=torch.empty((G, MAXMOVES), dtype=torch.float32, device=dev),
                   W=torch.empty((G, MAXMOVES), dtype=torch.float32, device=dev),
                   count=torch.empty(G, dtype=torch.int16, device=dev))
        self.ctx.call("cz_search_root_stats", *[out[k] for k in ("label", "N", "Q", "P", "W", "count")])
        return out

    def root_stats_host(self):
        st = self.root_stats()
        return dict(label=st["label"].cpu().numpy().view(np.uint16), N=st["N"].cpu().numpy(), Q=st["Q"].cpu().numpy(),
                    P=st["P"].cpu().numpy(), W=st["W"].cpu().numpy(), count=st["count"].cpu().numpy().view(np.uint16))

    def lines(self, n_lines=1, max_len=16, allowed=None):
        """Principal variations (cz_search_lines): for every tree the lines that start at its n_lines most visited root
        candidates — the root's children whose label is set in allowed [G, 66] int32 (a move set as Rules.movegen_kingsafe
        returns it; None: all children) — and follow the most visited child below them, every tie to the earlier child.  Call it
        between complete steps.  -> dict of device tensors: moves int16 (u16 bits, 0xFFFF padding) [G, n_lines, max_len],
        visits int32 and q float32 of the same shape, len int16 [G, n_lines].  Line 0's first move is the greedy move."""
        G, dev = self.G, self.dev
        n_lines, max_len = int(n_lines), int(max_len)
        allowed = self.ctx.tensor(allowed, torch.int32)
        assert allowed is None or allowed.shape == (G, _lib.MASK_WORDS), "allowed is a [G, 66] mask"
        shape = (G, max(n_lines, 0), max(max_len, 0))
        out = dict(moves=torch.empty(shape, dtype=torch.int16, device=dev), visits=torch.empty(shape, dtype=torch.int32, device=dev),
                   q=torch.empty(shape, dtype=torch.float32, device=dev), len=torch.empty(shape[:2], dtype=torch.int16, device=dev))
        self.ctx.call("cz_search_lines", allowed, n_lines, max_len, out["moves"], out["visits"], out["q"], out["len"])
        return out

    def lines_host(self, n_lines=1, max_len=16, allowed=None):
        ln = self.lines(n_lines, max_len, allowed)
        return dict(moves=ln["moves"].cpu().numpy().view(np.uint16), visits=ln["visits"].cpu().numpy(), q=ln["q"].cpu().numpy(),
                    len=ln["len"].cpu().numpy().view(np.uint16))

    def advance(self, played):
        if not torch.is_tensor(played):
            played = np.asarray(played, np.uint16)   # labels as u16 bits (0xFFFF: no move)
        self.ctx.call("cz_search_advance", self.ctx.tensor(played, torch.int16))

    def advance_ready(self, thr, next_thr, start_boards, start_side, start_rr=None, banked=None, reloaded=None):
        """The greedy driver of a long search loop, all on the device (cz_search_pick_ready -> cz_search_advance ->
        cz_search_reload_finished): every tree that has completed thr[g] simulations (int32 [G] device tensor, set to
        next_thr for the trees that move) plays its most visited root child; games that are then over restart from
        start_boards / start_side / start_rr.  banked / reloaded: int64 device scalars accumulating the simulations of the
        searches closed and the games restarted.  Returns the (played, ready) device tensors of this call."""
        G, dev = self.G, self.dev
        if getattr(self, "_ar", None) is None or self._ar[0].numel() != G:
            self._ar = (torch.empty(G, dtype=torch.int16, device=dev), torch.empty(G, dtype=torch.uint8, device=dev))
        played, ready = self._ar
        assert thr.dtype == torch.int32 and thr.is_cuda and thr.numel() == G
        self.ctx.call("cz_search_pick_ready", thr, int(next_thr), played, ready, banked)
        self.ctx.call("cz_search_advance", played)
        self.ctx.call("cz_search_reload_finished", ready, played, start_boards, start_side, start_rr, reloaded)
        return played, ready

    def status(self):
        G, dev = self.G, self.dev
        st, nodes, sims, depth = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(4))
        self.ctx.call("cz_search_status", st, nodes, sims, depth)
        return st, nodes, sims, depth

    def root_state(self):
        G, dev = self.G, self.dev
        b = torch.empty((G, NSQ), dtype=torch.uint8, device=dev)
        s = torch.empty(G, dtype=torch.uint8, device=dev)
        rr = torch.empty(G, dtype=torch.int32, device=dev)
        self.ctx.call("cz_search_root_state", b, s, rr)
        return b, s, rr

    def tree_dump(self, g, max_records=1 << 20):
        out = np.zeros((max_records, 7), np.int32)
        n = self.ctx.call("cz_search_tree_dump", int(g), out.ctypes.data, int(max_records))
        if n > max_records:
            raise _lib.CchessHipError("tree_dump: %d records > %d" % (n, max_records))
        return out[:n].copy()

    # -- the hot loop ------------------------------------------------------------------------------
    def step(self, forward, mode=1, active=None, tap=None, pre_net=None):
        """One lock-step simulation for every tree: select -> forward(planes) -> expand_backup.
        `forward` maps the device planes tensor to (logits [G,2086], value [G,1]) device tensors; if it is a
        PolicyValueNet with the fused hip backend (has `search_eval`) and width is 1, the policy FC is evaluated
        inside the expansion for the legal moves only (expand_backup_fc) and no logits tensor exists at all.
        tap (parity tests, bench events): called as tap(planes, z_or_logits, value) between the net and the expansion —
        the tensors are the ones the expansion kernel is about to read; pre_net() is called between select and the net."""
        net = getattr(forward, "__self__", forward)
        fused = self.width == 1 and getattr(net, "search_eval", None) is not None and net.fused_search
        compact = fused and self.compact   # terminal / drawn / parked trees cost the net nothing
        planes, n_rows = self.select_compact(mode, active) if compact else (self.select(mode, active)[0], None)
        if pre_net is not None:
            pre_net()
        out, value = net.search_eval(planes, n_rows) if fused else forward(planes)   # z [G,90,3] on the fused path, else logits
        if tap is not None:
            tap(planes, out, value)
        if fused:
            self.expand_backup_fc(out, value, net.pfc_w_rows, net.pfc_b_f32, compact=compact)
        else:
            self.expand_backup(out, value)

    def _active_bool(self, active):
        """The active mask as a bool device tensor for the host-side liveness tests of search(): None, a tensor / array,
        or a raw device pointer (what SelfPlay hands over in parking mode: cz_selfplay_active) — that one is downloaded."""
        if active is None:
            return None
        if isinstance(active, C.c_void_p):
            active = self.ctx.download(active, np.uint8, self.G)
        return torch.as_tensor(active).to(self.dev).bool()

    def _any_below(self, target, act):
        """Is any live (and active) tree still below `target` simulations?  (synchronises)"""
        st, _, sims, _ = self.status()
        live = (st & ~8) == 0
        if act is not None:
            live = live & act
        return bool(((sims < target) & live).any().item())

    def search(self, forward, playouts, active=None, root_done=False):
        """MCTS_tree.main (main.py:473-493) for all trees: expand unexpanded roots, then EXACTLY `playouts` simulations
        per (active, unparked) tree.  With width k > 1 up to k simulations are in flight per tree and step; a descent
        that runs into a pending expansion is abandoned (see k_select_k), so a step can complete fewer than k — the
        per-tree budget (cz_search_set_sim_target) and a few extra steps make up for it.  Returns the number of steps.
        root_done=True: the caller has already run the mode-0 step (root expansion).
        (Round 6 replayed the k-wide lock-step as one captured HIP graph for the --mode play shape — one tree, 16 simulations in
        flight — and measured no gain, 0.407 against 0.410 ms per lock-step: the step is five SERIAL small launches on the GPU, a
        203 us trunk for 16 positions and a k-wide select / expand that walk their 16 descents one after the other in one wave,
        not host time; the capture was removed again.)"""
        playouts = int(playouts)
        if not root_done:
            self.step(forward, mode=0, active=active)
        if self.width == 1 and self.terminal_extra == 0:
            for _ in range(playouts):
                self.step(forward, mode=1, active=active)
            return playouts
        if self.width == 1:
            # terminal simulations complete inside the select launches: a tree needs one lock-step per simulation that
            # needs the net, so the search is over when every tree has counted `playouts` (checked every 32 steps)
            base = self.status()[2]
            act = self._active_bool(active)   # parked / inactive slots neither decide the schedule nor keep the loop alive
            if act is not None:
                if not bool(act.any().item()):
                    return 0
                base = base[act]
            if not bool((base == base[0]).all().item()):   # stacked searches on unequal counters: the plain schedule
                extra = self.terminal_extra
                self.set_terminal_extra(0)
                try:
                    for _ in range(playouts):
                        self.step(forward, mode=1, active=active)
                finally:
                    self.set_terminal_extra(extra)
                return playouts
            target = int(base[0].item()) + playouts
            steps = 0
            self.set_sim_target(target)
            try:
                while steps < playouts:
                    for _ in range(min(32, playouts - steps)):
                        self.step(forward, mode=1, active=active)
                        steps += 1
                    if not self._any_below(target, act):
                        break
            finally:
                self.set_sim_target(0)
            return steps
        base = self.status()[2].clone()      # searches may be stacked on one root: the target is relative
        self.set_sim_target(0)
        # per-tree targets differ only if `base` does; the kernel takes one number, so stacked searches on trees with
        # different counters fall back to the unbudgeted schedule for the bulk and finish one simulation at a time
        uniform = bool((base == base[0]).all().item())
        target = int(base[0].item()) + playouts
        steps = 0
        try:
            if uniform:
                self.set_sim_target(target)
            one = lambda: self.step(forward, mode=1, active=active)
            n = (playouts + self.width - 1) // self.width
            for _ in range(n):
                one()
            steps = n
            if uniform:
                # the shortfall of abandoned descents: usually 1-3 steps — but behind a FRESH root every descent of a step picks the
                # same child (the reference never updates the root's N, quirk Q2: U = 0 there, and its virtual loss leaves Q alone),
                # so all but one are abandoned and a step completes ONE simulation: up to `playouts` steps, like the reference's
                # sixteen coroutines queueing behind one expansion (round 6: the cap of 4 n + 8 extra steps ended such a search short)
                act = self._active_bool(active)
                while steps < 5 * playouts + 8:
                    if not self._any_below(target, act):
                        break
                    one()
                    steps += 1
        finally:
            self.set_sim_target(0)
        return steps
