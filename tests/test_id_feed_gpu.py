"""The id-fed doc split on the GPU: rbr_doc_gather against torch, the recorded id-fed step and eval forward
against the doc-fed ones on the same pairs, and the trainer's `device_cache` against its doc-fed loop."""
import json
import math
import types

import numpy as np
import pytest
import torch

import make_dataset
import synth
from helpers import quiet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(1.0, abs(b))


def _id_tables(U, I, L, V, seed):
    """synth-style Zipf documents keyed by id; row 0 is the all-pad document (make_dataset / meta.pkl convention)."""
    rng = np.random.default_rng(seed)
    u, i = synth._docs(rng, U, L, V), synth._docs(rng, I, L, V)
    u[0] = 0
    i[0] = 0
    return u, i


def _cache(u_docs, i_docs, V):
    from review_based_recommender_amd import data as D
    ds = types.SimpleNamespace(user_docs=u_docs.tolist(), item_docs=i_docs.tolist(), user_num=len(u_docs),
                               item_num=len(i_docs), vocab_size=V)
    return D.DeviceDocCache(ds, DEV)


def _zipf_ids(rng, n, rows):
    """Zipf(1.07) over the ids [0, rows): repeats, and id 0 now and then."""
    p = np.arange(1, rows + 1, dtype=np.float64) ** -1.07
    return torch.from_numpy(rng.choice(rows, size=n, p=p / p.sum()).astype(np.int64))


def _doc_fed(u_tab, i_tab, u_ids, i_ids, with_ids=True):
    """What DocDataset.collate_fn builds for the pairs, on the host."""
    ud, idc = torch.from_numpy(u_tab)[u_ids], torch.from_numpy(i_tab)[i_ids]
    if not with_ids:
        return ud, idc
    return ud, idc, ud != 0, idc != 0, u_ids.clone(), i_ids.clone()


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("L", [512, 50, 1023, 1])
@pytest.mark.parametrize("form", ["block", "separate", "docs_only"])
def test_doc_gather_matches_index_select(L, form):
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import _flat_layout, _flat_views
    from review_based_recommender_amd.data import _adjacent
    U, I = 1001, 777
    g = torch.Generator().manual_seed(L)
    ut = torch.randint(0, 40, (U, L), generator=g, dtype=torch.int32)       # ~1 token in 40 is the pad id 0
    it = torch.randint(0, 40, (I, L), generator=g, dtype=torch.int32)
    u_ids = torch.tensor([0, 5, 5, 1000, -1, U, 2 ** 40, 17, 999, 5, 3, 0], dtype=torch.int64)
    i_ids = torch.tensor([3, I, -1, 0, 776, 2 ** 40, 776, 776, 12, 1, 9, 0], dtype=torch.int64)
    B = u_ids.numel()
    uc = torch.where((u_ids >= 0) & (u_ids < U), u_ids, torch.zeros_like(u_ids))
    ic = torch.where((i_ids >= 0) & (i_ids < I), i_ids, torch.zeros_like(i_ids))
    n_bad = int((uc != u_ids).sum() + (ic != i_ids).sum())
    ref_docs = torch.cat([ut.index_select(0, uc), it.index_select(0, ic)]).long()
    RF.check_id_errors(DEV)                                                   # a clean record to start from
    ut_d, it_d, u_d, i_d = ut.to(DEV), it.to(DEV), u_ids.to(DEV), i_ids.to(DEV)
    if form == "block":          # the adjacent views of one block, as a recorded step's input slot lays them out
        like = [torch.empty(B, L, dtype=torch.int64)] * 2 + [torch.empty(B, L, dtype=torch.bool)] * 2 + \
               [torch.empty(B, dtype=torch.int64)] * 2
        layout = _flat_layout(like)
        flat = torch.full((layout[-1],), 0xAB, dtype=torch.uint8, device=DEV)
        v = _flat_views(flat, layout, like)
        outs = dict(docs=_adjacent(v[0], v[1]), masks=_adjacent(v[2], v[3]), ids=_adjacent(v[4], v[5]))
        docs, masks, ids = RF.doc_gather(u_d, i_d, ut_d, it_d, **outs)
        assert docs.data_ptr() == v[0].data_ptr() and masks.data_ptr() == v[2].data_ptr() and ids.data_ptr() == v[4].data_ptr()
    elif form == "separate":
        docs, masks, ids = RF.doc_gather(u_d, i_d, ut_d, it_d)
    else:                        # D-ATT: documents only
        docs, masks, ids = RF.doc_gather(u_d, i_d, ut_d, it_d, masks=None, ids=None)
        assert masks is None and ids is None
    torch.cuda.synchronize()
    assert docs.dtype == torch.int64 and docs.shape == (2 * B, L)
    assert torch.equal(docs.cpu(), ref_docs)
    if masks is not None:
        assert masks.dtype == torch.bool and torch.equal(masks.cpu(), ref_docs != 0)
        assert torch.equal(ids.cpu(), torch.cat([uc, ic]))
    rec = RF._id_err(DEV).cpu()
    assert int(rec[0]) == n_bad
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)                                                   # raised once; the record is clear again


# ------------------------------------------------------------------------------------------------ 2. the recorded step
def _deepconn(cfg, dedup):
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    m = quiet(DeepCoNNpp, cfg["U"], cfg["I"], cfg["V"], cfg["kz"], cfg["D"], cfg["H"], cfg["K"], cfg["L"], None, 0.0)
    m.load_state_dict(synth.deepconn_params(cfg, 0))
    m.validate_ids = False
    m.dedup_by_id = dedup
    return m.to(DEV).train()


def _datt(cfg):
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    c = cfg
    m = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.0, None)
    m.load_state_dict(synth.datt_params(cfg, 0, table_scale=0.5))
    m.validate_ids = False
    return m.to(DEV).train()


def _check_params(m_a, m_b, lr=2e-3):
    """helpers.check_params_after's gates: lr/2 max, 1e-4 RMS."""
    for (n, a), b in zip(m_a.named_parameters(), m_b.parameters()):
        d = (a.detach() - b.detach()).double()
        assert float(d.abs().max()) <= lr / 2, n
        assert float(d.pow(2).mean().sqrt()) <= 1e-4, n


def _paired_steps(make_model, cfg, U, I, with_ids, slots, n_steps=3, seed=5):
    """The doc-fed and the id-fed GraphedTrainStep from the same initial state over the same pairs: exact inputs, close
    outcomes.  Returns (doc-fed launches, id-fed launches)."""
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    B, L, V = cfg["B"], cfg["L"], cfg["V"]
    u_tab, i_tab = _id_tables(U, I, L, V, seed)
    cache = _cache(u_tab, i_tab, V)
    rng = np.random.default_rng(seed + 1)
    pairs = [(_zipf_ids(rng, B, U), _zipf_ids(rng, B, I), torch.from_numpy(rng.integers(1, 6, B).astype(np.float32)))
             for _ in range(n_steps + 1)]
    m_d, m_i = make_model(), make_model()
    o_d = make_optimizer(m_d, capturable=True, hip_clip_adam=True)
    o_i = make_optimizer(m_i, capturable=True, hip_clip_adam=True)
    u0, i0, r0 = pairs[-1]                                      # recorded on pairs that are not replayed
    st_d = GraphedTrainStep(m_d, o_d, [t.to(DEV) for t in _doc_fed(u_tab, i_tab, u0, i0, with_ids)], r0.to(DEV), slots=slots,
                            keep_graph=True)
    st_i = GraphedTrainStep.from_ids(m_i, o_i, cache, u0.to(DEV), i0.to(DEV), r0.to(DEV), with_ids=with_ids, slots=slots,
                                     keep_graph=True)
    for a, b in zip(m_d.parameters(), m_i.parameters()):
        assert torch.equal(a, b)
    for k, (u, i, r) in enumerate(pairs[:n_steps]):
        s = k % slots
        st_d.stage(s, [t.to(DEV) for t in _doc_fed(u_tab, i_tab, u, i, with_ids)], r.to(DEV))
        st_i.stage(s, (u, i), r)                                 # host ids: one host-to-device copy of the id block
        ld, gd, pd = st_d(slot=s)
        li, gi, pi = st_i(slot=s)
        torch.cuda.synchronize()
        for a, b in zip(st_i.slot_batch(s), st_d.slot_batch(s)):     # what the gather wrote = what the loader staged
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert _rel(li, ld) <= 1e-5 and _rel(gi, gd) <= 1e-5, (k, float(li), float(ld), float(gi), float(gd))
        assert float((pi - pd).abs().max()) <= 1e-5 * max(1.0, float(pd.abs().max())), k
    _check_params(m_d, m_i)
    return st_d.kernel_launches(), st_i.kernel_launches()


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("dedup", [False, True])
def test_id_fed_step_matches_doc_fed_cfg2(slots, dedup, conv_mode):
    cfg = synth.DEEPCONN_CFGS["cfg2"]
    n_d, n_i = _paired_steps(lambda: _deepconn(cfg, dedup), cfg, cfg["U"], cfg["I"], True, slots)
    if n_d is not None and n_i is not None:
        assert n_i == n_d + 1, (n_d, n_i)


@pytest.mark.parametrize("name", ["small", "cfg4"])
def test_id_fed_step_matches_doc_fed_datt(name):
    cfg = synth.DATT_CFGS[name]
    n_d, n_i = _paired_steps(lambda: _datt(cfg), cfg, 1001, 777, False, 1 if name == "cfg4" else 2)
    if n_d is not None and n_i is not None:
        assert n_i == n_d + 1, (n_d, n_i)


# ------------------------------------------------------------------------------------------------ 4. eval forward
def test_id_fed_eval_forward_matches_doc_fed(capsys):
    from review_based_recommender_amd.train_step import GraphedForward
    cfg = synth.DEEPCONN_CFGS["cfg1"]
    B, L, V, U, I = cfg["B"], cfg["L"], cfg["V"], cfg["U"], cfg["I"]
    u_tab, i_tab = _id_tables(U, I, L, V, 9)
    cache = _cache(u_tab, i_tab, V)
    m = _deepconn(cfg, False).eval()
    rng = np.random.default_rng(10)
    u0, i0 = _zipf_ids(rng, B, U), _zipf_ids(rng, B, I)
    g_d = GraphedForward(m, [t.to(DEV) for t in _doc_fed(u_tab, i_tab, u0, i0)])
    g_i = GraphedForward.from_ids(m, cache, u0.to(DEV), i0.to(DEV))
    bit_equal = True
    for _ in range(3):
        u, i = _zipf_ids(rng, B, U), _zipf_ids(rng, B, I)
        p_d = g_d([t.to(DEV) for t in _doc_fed(u_tab, i_tab, u, i)]).clone()
        p_i = g_i((u.to(DEV), i.to(DEV))).clone()
        torch.cuda.synchronize()
        assert float((p_i - p_d).abs().max()) <= 1e-6 * max(1.0, float(p_d.abs().max()))
        bit_equal &= torch.equal(p_i, p_d)
    with capsys.disabled():
        print(f"\nid-fed eval forward bit-equal to the doc-fed one: {bit_equal}")


# ------------------------------------------------------------------------------------------------ 5. trainer
def _cfg(tmp_path, kind, data_dir, **extra):
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": kind, "parallel": False, "kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12,
           "latent_dim": 4, "dropout": 0.0, "arch": "CNN", "use_pretrain": False, "epochs": 2, "batch_size": 20, "lr": 0.002,
           "max_grad_norm": 5.0, "patience": 5, "l_window_size": 5, "l_out_size": 8, "g_out_size": 4, "emb_size": 12,
           "hidden_size_1": 10, "hidden_size_2": 5, "fast_step": True, "shuffle": False, "record_steps": True}
    cfg.update(extra)
    path = tmp_path / f"{kind}_{int(cfg.get('device_cache', False))}.json"
    path.write_text(json.dumps(cfg))
    return str(path)


@pytest.mark.parametrize("kind", ["deepconn", "dual_att"])
def test_trainer_device_cache_follows_the_doc_fed_trainer(tmp_path, kind):
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)                       # 96 train / 32 valid pairs: ragged last batches of 16 and 12
    runs = {}
    for cache in (False, True):
        torch.manual_seed(0)
        exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, device_cache=cache)), uid=f"c{int(cache)}")
        assert (exp.cache is not None) == cache
        rmse = []
        for e in range(exp.args.epochs):
            exp.train_one_epoch(e)
            exp.valid_one_epoch()
            rmse.append(exp.last_valid_rmse)
        runs[cache] = ([float(x) for x in exp.step_losses], rmse, exp.valid_count)
    (l_d, r_d, n_d), (l_i, r_i, n_i) = runs[False], runs[True]
    assert len(l_d) == len(l_i) == 2 * 5
    for k, (a, b) in enumerate(zip(l_i, l_d)):
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    for a, b in zip(r_i, r_d):
        assert abs(a - b) <= 1e-5 * abs(b) and math.isfinite(a), (a, b)
    assert n_i == n_d == 32
