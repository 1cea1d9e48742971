"""The two-launch prepare stage on a kept workspace (rbr_textcnn_prod_prepare_ids_kept: list state zero on entry, zero on
exit) against the self-initialising three-launch chain (rbr_textcnn_prod_prepare_ids) on the same inputs.

Equal as integers: row_of_token, tok_of_row[:count], count, the row mask, the cleaned ids, err (its count; see _equal), the slab flags, the slab work
list as a sorted set with its count; equal bits: pooled features and argmax of the forward that follows.

Shapes: V = 257 and 1000 (no multiple of 256 or 16), n_docs x L = 2 x 33 (66 tokens: fewer than one block, a partial second
slab) and 5 x 64 (320: more than one block).  The three-launch reference runs on a workspace filled with 0xAB bytes.

The plain chain (rbr_textcnn_prod_prepare: no id sets; its mark and compaction launches are the list backward's too) is compared
with the three-launch ids chain in the same way, on the clean ids that chain produced."""
import ctypes as C
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 8
KZ, CH = (3, 5), (5, 6)
SHAPES = [(V, n, L) for V in (257, 1000) for (n, L) in ((2, 33), (5, 64))]
CASES = ("distinct", "one_token", "all_masked", "bad_ids", "no_mask")


@pytest.fixture(autouse=True)
def _product_conv():
    from review_based_recommender_amd import _lib
    _lib.lib().rbr_set_conv_mode(2)
    os.environ.pop("RBR_PREP_TWO_LAUNCH", None)
    yield
    _lib.lib().rbr_set_conv_mode(0)


def _case(case, V, n_docs, L, seed=0):
    """(raw ids [n_docs, L] int64, mask [n_docs, L] bool or None) on the host."""
    g = torch.Generator().manual_seed(100 + seed)
    n = n_docs * L
    ids = torch.randint(1, V, (n_docs, L), generator=g)
    mask = torch.rand(n_docs, L, generator=g) < 0.7
    mask[0, :3] = True
    if case == "distinct":            # every token another one (all table rows in use where the batch is larger than the table)
        ids = (torch.randperm(max(n, V), generator=g)[:n] % V).view(n_docs, L)
        mask[:] = True
    elif case == "one_token":
        ids[:] = 7
    elif case == "all_masked":
        mask[:] = False
    elif case == "bad_ids":
        flat = ids.view(-1)
        flat[0], flat[5], flat[n - 1], flat[n // 2], flat[9] = -1, V, V + 100, 1 << 40, -(1 << 40)
        mask.view(-1)[[0, 5, n - 1, n // 2]] = True
    elif case == "no_mask":
        mask = None
    return ids, mask


class _Rec:
    pass


@functools.lru_cache(maxsize=None)
def _params(V):
    g = torch.Generator().manual_seed(V)
    table = (torch.rand(V, D, generator=g) * 2 - 1).to(DEV)
    ws = [((torch.rand(c, D, k, generator=g) * 2 - 1) * 0.3).to(DEV) for k, c in zip(KZ, CH)]
    bs = [((torch.rand(c, generator=g) * 2 - 1) * 0.3).to(DEV) for c in CH]
    return table, ws, bs


def _forward(V, ids_raw, mask, kept, prod_ws=None, static=None, clean_from=None):
    """prepare -> table -> pool -> finalize through functional's stage sequence; everything the comparison reads, as host
    tensors.  kept: a workspace from functional's kept workspaces (or `prod_ws`, a tensor carrying one) and the two-launch
    stage; else a 0xAB-filled workspace and the three-launch stage.  static: (raw, extra, mask) device buffers to use.
    clean_from: the clean ids of an earlier call -- the PLAIN chain (rbr_textcnn_prod_prepare: no id sets, no range check)
    runs on them, on a 0xAB-filled workspace."""
    from review_based_recommender_amd import _lib, functional as RF
    L_ = _lib.lib()
    dev = torch.device(DEV)
    n_docs, L = ids_raw.shape
    table, ws, bs = _params(V)
    if static is None:
        raw = ids_raw.to(DEV).contiguous()
        extra = torch.tensor([0, 4, 5, -2, 3, 1 << 33, 2], dtype=torch.int64, device=DEV)      # a set that is no conv token: limit 5
        mask8 = None if mask is None else mask.to(DEV).to(torch.uint8).contiguous()
    else:
        raw, extra, mask8 = static
    clean = torch.full((raw.numel() + extra.numel(),), -77, dtype=torch.int64, device=DEV)
    ids = clean[:raw.numel()].view(n_docs, L)
    err = torch.zeros(4, dtype=torch.int64, device=DEV)
    arr = (_lib.IdSet * 2)()
    arr[0] = _lib.IdSet(raw.data_ptr(), ids.data_ptr(), raw.numel(), V, 0)
    arr[1] = _lib.IdSet(extra.data_ptr(), clean[raw.numel():].data_ptr(), extra.numel(), 5, 1)
    desc = RF._conv_desc(table, n_docs, L, ws, RF.PAD_SAME, RF.ACT_RELU, 0)
    rec = RF._conv_fwd_buffers(_Rec(), desc, dev, kept=kept and prod_ws is None)
    assert rec.prod_ws is not None
    if prod_ws is not None:
        rec.prod_ws = prod_ws
    if kept:
        assert getattr(rec.prod_ws, "_kept", None) is not None
    else:
        rec.prod_ws.fill_(0xAB)
        rec.pidx.fill_(-5)
    st = _lib.current_stream()
    if clean_from is not None:
        assert not kept
        ids = clean_from[:raw.numel()].view(n_docs, L)
    id_sets = None if clean_from is not None else (2, arr, err.data_ptr())
    RF._prod_forward(desc, rec, table, ids, mask8, None, ws, st, id_sets=id_sets)
    RF._pool_finalize(desc, rec, bs, st)
    out = _Rec()
    out.rec, out.desc, out.clean, out.err = rec, desc, clean, err
    out.keep = (raw, extra, mask8, table, ws, bs, arr)
    return out


def _read(out, V):
    """Host copies of what the issue's comparison names (call after a synchronize)."""
    from review_based_recommender_amd import _lib
    L_ = _lib.lib()
    rec, desc = out.rec, out.desc
    wsb = rec.prod_ws
    rot, nrows, tor, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
    assert L_.rbr_textcnn_token_list(C.byref(desc), wsb.data_ptr(), C.byref(rot), C.byref(nrows), C.byref(tor), C.byref(cap)) == 0
    base = wsb.data_ptr()

    def view(ptr, nbytes, dtype):
        o = ptr - base
        return wsb[o:o + nbytes].view(dtype).cpu()

    count = int(view(nrows.value, 4, torch.int32)[0])
    off = (C.c_int64 * 6)()
    assert L_.rbr_textcnn_prod_list_state(C.byref(desc), off) == 0
    total_wt = desc.n_docs * ((desc.L + 31) // 32)
    sched = rec.pidx[rec.pidx.numel() - 64 - 2 * total_wt:].cpu()
    n_slabs = int(sched[2 * total_wt])
    r = dict(row_of_token=view(rot.value, 4 * V, torch.int32), count=count,
             tok_of_row=view(tor.value, 8 * cap.value, torch.int64)[:count],
             row_mask=wsb[off[2]:off[2] + off[3]].cpu(), clean=out.clean.cpu(), err=out.err.cpu(),
             flags=sched[:total_wt], n_slabs=n_slabs, slabs=torch.sort(sched[total_wt:total_wt + n_slabs]).values,
             other_counters=sched[2 * total_wt + 1:], feat=rec.feat.cpu(), argmax=rec.argmax.cpu())
    state = torch.cat([wsb[off[0]:off[0] + off[1]], wsb[off[4]:off[4] + off[5]]]).cpu()
    return r, state


def _equal(a, b, what=""):
    for k in a:
        if k == "count" or k == "n_slabs":
            assert a[k] == b[k], (what, k, a[k], b[k])
        elif k == "err":
            # err[0] counts the offenders; err[1], err[2] name ANY ONE of them (a benign race by design, in either chain): equal
            # counts, and each record a real offender of its set
            assert int(a[k][0]) == int(b[k][0]) and int(a[k][3]) == int(b[k][3]), (what, k)
            for e in (a[k], b[k]):
                assert int(e[0]) == 0 or (int(e[2]) in (0, 1) and not 0 <= int(e[1]) < (5 if int(e[2]) else a["row_of_token"].numel()))
        else:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("V,n_docs,L", SHAPES)
def test_two_launches_equal_three(V, n_docs, L, case):
    ids, mask = _case(case, V, n_docs, L)
    new = _forward(V, ids, mask, kept=True)
    old = _forward(V, ids, mask, kept=False)
    torch.cuda.synchronize()
    rn, state = _read(new, V)
    ro, _ = _read(old, V)
    _equal(rn, ro, case)
    assert int(state.count_nonzero()) == 0, "the list state is not zero after the call"
    n_tok = n_docs * L
    if case == "all_masked":
        assert rn["count"] == 0 and int((rn["row_of_token"] >= 0).sum()) == 0 and int(rn["row_mask"].sum()) == 0
    if case == "one_token":
        assert rn["count"] == 1 and int(rn["tok_of_row"][0]) == 7
    if case == "distinct":
        assert rn["count"] == min(n_tok, V)
    if case == "bad_ids":
        c = rn["clean"][:n_tok]
        assert int(c.min()) >= 0 and int(c.max()) < V and int(c[0]) == 0 and int(c[5]) == 0 and int(c[n_tok - 1]) == 0
        assert int(rn["err"][0]) == 5 + 3           # five bad token ids, three bad ids in the other set
    else:
        assert int(rn["err"][0]) == 3
    assert int(rn["row_mask"].sum()) == rn["count"] and int(rn["row_mask"][:rn["count"]].sum()) == rn["count"]


@pytest.mark.parametrize("case", ("distinct", "one_token", "all_masked", "no_mask"))
@pytest.mark.parametrize("V,n_docs,L", SHAPES)
def test_plain_chain_equals_ids_chain(V, n_docs, L, case):
    """The plain chain (rbr_textcnn_prod_prepare, no id sets: zero | mark + scan | compact + pack -- the launches it shares with
    the list backward) on the clean ids that the three-launch ids chain produced, both on 0xAB-filled workspaces: the same list,
    work list and forward, integer for integer.  `clean` and `err` are not compared: the plain chain produces neither."""
    ids, mask = _case(case, V, n_docs, L)
    ref = _forward(V, ids, mask, kept=False)
    torch.cuda.synchronize()
    plain = _forward(V, ids, mask, kept=False, clean_from=ref.clean)
    torch.cuda.synchronize()
    rr, _ = _read(ref, V)
    rp, _ = _read(plain, V)
    assert torch.equal(rr["clean"][:n_docs * L], ids.view(-1)), "the case's ids are clean: the chains saw the same tokens"
    for r in (rr, rp):
        del r["clean"], r["err"]
    _equal(rp, rr, case)
    assert rp["count"] == {"distinct": min(n_docs * L, V), "one_token": 1, "all_masked": 0}.get(case, rp["count"])


@pytest.mark.parametrize("V,n_docs,L", SHAPES)
def test_three_batches_in_a_row_on_one_workspace(V, n_docs, L):
    """One zero-initialised workspace, three different batches: each equals the three-launch chain on a fresh workspace and
    leaves the list state zero."""
    held = None
    for k, case in enumerate(("distinct", "bad_ids", "one_token")):
        ids, mask = _case(case, V, n_docs, L, seed=k)
        new = _forward(V, ids, mask, kept=True)
        if held is None:
            held = new.rec.prod_ws._kept
        assert new.rec.prod_ws._kept is held, "the second call did not get the first call's workspace back"
        old = _forward(V, ids, mask, kept=False)
        torch.cuda.synchronize()
        rn, state = _read(new, V)
        ro, _ = _read(old, V)
        _equal(rn, ro, case)
        assert int(state.count_nonzero()) == 0
        del new, old


def test_recorded_chain_replayed_on_two_batches():
    """The two-launch chain recorded into a graph (its workspace owned by the recording) and replayed twice, on two batches
    staged in turn, against the three-launch chain run eagerly on the same batches."""
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import _capture_stream
    V, n_docs, L = 257, 5, 64
    batches = [_case("bad_ids", V, n_docs, L, seed=1), _case("distinct", V, n_docs, L, seed=2)]
    warm = _forward(V, *batches[0], kept=True)                # sizes the kept workspaces of the device
    torch.cuda.synchronize()
    del warm
    raw = torch.zeros(n_docs, L, dtype=torch.int64, device=DEV)
    extra = torch.tensor([0, 4, 5, -2, 3, 1 << 33, 2], dtype=torch.int64, device=DEV)
    mask8 = torch.zeros(n_docs, L, dtype=torch.uint8, device=DEV)
    raw.copy_(batches[0][0]); mask8.copy_(batches[0][1])
    cs = _capture_stream(torch.device(DEV))
    owned = []
    graph = torch.cuda.CUDAGraph()
    with RF.kept_ws_owner(owned), torch.cuda.graph(graph, stream=cs):
        rec = _forward(V, batches[0][0], None, kept=True, static=(raw, extra, mask8))
    assert len(owned) == 1 and rec.rec.prod_ws._kept is owned[0]
    for ids, mask in batches:
        raw.copy_(ids); mask8.copy_(mask)
        rec.err.zero_()
        graph.replay()
        torch.cuda.synchronize()
        rn, state = _read(rec, V)
        old = _forward(V, ids, mask, kept=False)
        torch.cuda.synchronize()
        ro, _ = _read(old, V)
        _equal(rn, ro)
        assert int(state.count_nonzero()) == 0


def test_owner_clears_the_workspace_after_a_failed_call():
    """A call that returns an error (a token set whose limit exceeds the table: RBR_ERR_BAD_ARG) leaves the workspace marked
    dirty; whatever state it holds -- here: marks and counters scribbled over -- is cleared before the next use, which is
    correct."""
    from review_based_recommender_amd import _lib, functional as RF
    V, n_docs, L = 257, 2, 33
    ids, mask = _case("distinct", V, n_docs, L)
    first = _forward(V, ids, mask, kept=True)
    torch.cuda.synchronize()
    ws = first.rec.prod_ws._kept
    desc, rec = first.desc, first.rec
    raw, extra, mask8, table, wts, bs, arr = first.keep
    bad = (_lib.IdSet * 2)()
    bad[0] = _lib.IdSet(raw.data_ptr(), first.clean.data_ptr(), raw.numel(), V + 1, 0)      # limit above the table
    bad[1] = arr[1]
    with pytest.raises(RuntimeError):
        RF._prod_forward(desc, rec, table, first.clean[:raw.numel()].view(n_docs, L), mask8, None, wts, _lib.current_stream(),
                         id_sets=(2, bad, first.err.data_ptr()))
    assert ws.dirty
    for o, n in ws.state:
        ws.buf[o:o + n].fill_(0x5A)          # what a chain that stopped between its launches may leave behind, and worse
    del first, rec
    again = _forward(V, ids, mask, kept=True)
    assert again.rec.prod_ws._kept is ws and not ws.dirty
    old = _forward(V, ids, mask, kept=False)
    torch.cuda.synchronize()
    rn, state = _read(again, V)
    ro, _ = _read(old, V)
    _equal(rn, ro)
    assert int(state.count_nonzero()) == 0


def test_switch_off_takes_the_three_launch_chain():
    from review_based_recommender_amd import functional as RF
    os.environ["RBR_PREP_TWO_LAUNCH"] = "0"
    try:
        V, n_docs, L = 257, 2, 33
        table, ws, _ = _params(V)
        desc = RF._conv_desc(table, n_docs, L, ws, RF.PAD_SAME, RF.ACT_RELU, 0)
        rec = RF._conv_fwd_buffers(_Rec(), desc, torch.device(DEV), kept=True)
        assert rec.prod_ws is not None and getattr(rec.prod_ws, "_kept", None) is None
    finally:
        os.environ.pop("RBR_PREP_TWO_LAUNCH", None)
