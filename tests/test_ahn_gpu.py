"""AHN on the HIP path against the fixtures the reference wrote (tests/golden/make_golden_ahn.py: the reference's AHN on the CPU in
float64), with the checks and tolerances tests/test_narre_datt_gpu.py applies to NARRE's fixtures."""
import pytest
import torch

import synth_ahn
from helpers import check_grads, check_params_after, golden, max_err, quiet

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4
DEV = "cuda:0"
NAMES = ("tiny", "small")


def _params(g):
    return {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}


def _model(c, g, **kw):
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    kw.setdefault("dropout", 0.0)
    m = quiet(AHN, c["E"], c["H"], c["K"], c["U"], c["I"], c["V"], None, item_review_num=c["R"], **kw)
    m.load_state_dict(_params(g))
    return m.to(DEV)


def _batch(g):
    return tuple(torch.from_numpy(g["in/" + k]).to(DEV) for k in synth_ahn.FORWARD_KEYS), torch.from_numpy(g["in/ratings"]).to(DEV)


@pytest.mark.parametrize("name", NAMES)
def test_ahn_matches_reference(golden_dir, name):
    from review_based_recommender_amd.train_step import make_optimizer, train_step
    g = golden(golden_dir, "ahn_" + name)
    c = synth_ahn.AHN_CFGS[name]
    model = _model(c, g)
    args, ratings = _batch(g)
    model.eval()
    with torch.no_grad():
        pred, usw, isw, urw, irw = model(*args)
        u_sents, i_sents = model.encode_sentences(args[0], args[1], args[4], args[5])
    assert pred.shape == (c["B"],) and usw.shape == (c["B"], c["R"], c["S"]) and urw.shape == (c["B"], c["R"])
    assert max_err(u_sents.cpu().view(-1, c["H"]).numpy(), g["user_sents"]) <= 1e-5
    assert max_err(i_sents.cpu().view(-1, c["H"]).numpy(), g["item_sents"]) <= 1e-5
    assert max_err(pred.cpu().numpy(), g["pred_eval"]) <= FWD_TOL
    for got, key in ((usw, "user_sent_weights"), (isw, "item_sent_weights"), (urw, "user_review_weights"), (irw, "item_review_weights")):
        assert max_err(got.cpu().numpy(), g[key]) <= 1e-5, key

    # eval() is deterministic bit for bit
    with torch.no_grad():
        again = model(*args)
    for a, b in zip((pred, usw, isw, urw, irw), again):
        assert torch.equal(a, b)

    model.train()
    out = model(*args)[0]
    assert max_err(out.detach().cpu().numpy(), g["pred"]) <= FWD_TOL
    loss = torch.nn.functional.mse_loss(out, ratings)
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    loss.backward()
    check_grads({k: p.grad for k, p in model.named_parameters()}, g)
    model.zero_grad()
    opt = make_optimizer(model, hip_clip_adam=True)
    for step in range(3):
        loss, gnorm, _ = train_step(model, opt, args, ratings)
        if step == 0:
            assert abs(float(loss) - float(g["loss"])) <= 1e-4
            assert abs(float(gnorm) - float(g["gnorm"])) <= 2e-4 * float(g["gnorm"])
        if step in (0, 2):
            check_params_after(model, g, f"after{step + 1}")


def test_sides_of_different_width_take_two_encoder_calls(golden_dir):
    """iw_num != uw_num: the sides cannot share a batch; the item side padded by two more (empty) word columns gives the same
    sentences as the shared batch."""
    g = golden(golden_dir, "ahn_tiny")
    c = synth_ahn.AHN_CFGS["tiny"]
    model = _model(c, g).eval()
    args, _ = _batch(g)
    wide = torch.cat([args[1], torch.zeros(*args[1].shape[:3], 2, dtype=torch.int64, device=DEV)], dim=3)
    with torch.no_grad():
        a = model(*args)
        b = model(args[0], wide, *args[2:])
    for x, y in zip(a, b):
        assert max_err(x.cpu().numpy(), y.cpu().numpy()) <= 1e-6


def test_state_dict_round_trip_from_a_reference_layout_checkpoint(golden_dir, tmp_path):
    g = golden(golden_dir, "ahn_tiny")
    c = synth_ahn.AHN_CFGS["tiny"]
    sd = _params(g)
    path = tmp_path / "ahn.pt"
    torch.save(sd, path)
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    m = quiet(AHN, c["E"], c["H"], c["K"], c["U"], c["I"], c["V"], None, item_review_num=c["R"])
    m.load_state_dict(torch.load(path))
    m.to(DEV)
    back = m.state_dict()
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k].cpu(), sd[k]), k
    args, _ = _batch(g)
    m.eval()
    with torch.no_grad():
        assert max_err(m(*args)[0].cpu().numpy(), g["pred_eval"]) <= FWD_TOL


def test_rnn_dropout_is_one_multiplier_per_sentence_shared_over_time(golden_dir):
    """Train mode with rnn_dropout = 0.3 equals the same chain called by hand with the drawn multiplier."""
    from review_based_recommender_amd import functional as RF
    g = golden(golden_dir, "ahn_tiny")
    c = synth_ahn.AHN_CFGS["tiny"]
    model = _model(c, g, rnn_dropout=0.3).train()
    args, _ = _batch(g)
    n = 2 * c["B"] * c["R"] * c["S"]
    torch.manual_seed(11)
    out = model(*args)
    # the same draw again: the multiplier kernel is keyed by the device generator's seed and a call counter on the device
    seed, state = RF._drop_rng(torch.device(DEV))
    state[0] -= 1
    drop = RF.dropout_multiplier((n, c["E"]), 0.3, True, DEV)
    assert all(v == 0.0 or abs(v - 1 / 0.7) < 1e-6 for v in drop.unique().tolist())
    assert 0.1 < float((drop == 0).float().mean()) < 0.5
    u_sents, i_sents = model.encode_sentences(args[0], args[1], args[4], args[5], drop=drop)
    by_hand = model.aggregate(u_sents, i_sents, args[2], args[3], args[6], args[7], args[8], args[9])
    for a, b in zip(out, by_hand):
        assert torch.equal(a, b)
    # ... and it is the encoder on x * multiplier, the same multiplier at every time step
    ids = torch.cat([args[0].reshape(-1, c["W"]), args[1].reshape(-1, c["W"])])
    lens = torch.cat([args[4].reshape(-1), args[5].reshape(-1)])
    x = RF.embedding(model.word_embeddings.weight, ids, 0) * drop.unsqueeze(1)
    t_out = torch.cat([RF.lstm_t_out(args[4].reshape(-1), c["W"]).expand(n // 2), RF.lstm_t_out(args[5].reshape(-1), c["W"]).expand(n // 2)])
    pooled, _ = RF.bilstm_encode(x, model.word_encoder.lstm_params(), lens, pool=True, t_out=t_out)
    assert torch.equal(pooled[:n // 2].view_as(u_sents), u_sents) and torch.equal(pooled[n // 2:].view_as(i_sents), i_sents)
    model.eval()
    with torch.no_grad():
        a, b = model(*args), model(*args)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_seq2seq_encoder_forward_returns_the_trimmed_shape(golden_dir):
    import lstm_ref as R
    from review_based_recommender_amd.models.ahn.ahn_layers import Seq2SeqEncoder
    torch.manual_seed(3)
    enc = Seq2SeqEncoder(torch.nn.LSTM, 6, 5, bidirectional=True).to(DEV)
    x = torch.randn(7, 9, 6, device=DEV)
    lengths = torch.tensor([0, 4, 1, 6, 0, 2, 6], device=DEV)
    out = enc(x, lengths)
    assert out.shape == (7, 6, 10)
    ref = R.bilstm(x.cpu().double(), [p.detach().cpu().double() for p in enc.lstm_params()], lengths.cpu())
    assert float((out.detach().cpu().double() - ref[:, :6]).abs().max()) <= 2e-6
    assert float(out[lengths == 0].abs().sum()) == 0.0
    pooled = enc.encode_max(x, lengths)
    assert torch.equal(pooled, out.max(dim=1).values)
    assert enc(x, torch.zeros(7, dtype=torch.int64, device=DEV)).shape == (7, 1, 10)
