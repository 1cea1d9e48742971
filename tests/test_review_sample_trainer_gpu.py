"""The trainer's `sample_train_review`: one epoch of SimpleSiamese with sampled reviews from a pool wider than rv_num finishes,
logs, checkpoints and repeats itself under the same seeds; switched off, the key changes nothing."""
import os
import re

import pytest
import torch

import make_review_dataset
from test_review_feed_gpu import _cfg

pytestmark = pytest.mark.gpu


def _run(tmp_path, data_dir, tag, **extra):
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    torch.manual_seed(0)
    exp = ReviewExperiment("simple_siamese", parse_args(_cfg(tmp_path, "simple_siamese", data_dir, tag, device_reviews=True,
                                                             epochs=1, **extra)), uid=tag)
    exp.train_one_epoch(0)
    exp.valid_one_epoch()
    with open(exp.log_path) as f:
        log = f.read().splitlines()
    return exp, [float(x) for x in exp.step_losses], log


def test_trainer_trains_with_sampled_reviews_and_repeats_itself(tmp_path):
    from review_based_recommender_amd import data as D
    data_dir = str(tmp_path / "data")
    info = make_review_dataset.write_review_split(data_dir)      # 43 train pairs: two recorded steps and a ragged eager one
    kw = dict(sample_train_review=True, u_rv_num=2, i_rv_num=2, review_pool=6, seed=3, review_sample_seed=11)
    exp, losses, log = _run(tmp_path, data_dir, "s0", **kw)
    assert isinstance(exp.train_feed, D.SampledReviewFeed) and type(exp.eval_feed) is D.ReviewFeed
    assert (exp.train_feed.n_user, exp.train_feed.n_item, exp.train_feed.seed, exp.cache.pool) == (2, 2, 11, 6)
    assert exp.cache.user_pool_table.shape[1] == 7 and exp.cache.user_table.shape[1] == info["rv_num"] + 1
    assert len(losses) == 3 and all(l == l and abs(l) < 1e6 for l in losses)
    assert exp.train_feed.state.tolist() == [3, 0]               # one draw per step: the recording's warm-up used none up
    steps = [l for l in log if l.startswith("epoch: ")]
    assert len(steps) == 1 and re.match(r"epoch: 0/1, step: 2/3, loss: \d+\.\d{3}, rmse: \d+\.\d{3}, lr: 0.002, gnorm: ", steps[0])
    assert sum(l.startswith("valid loss: ") for l in log) == 1 and "sample_train_review: True" in log
    assert os.path.isfile(os.path.join(exp.out_dir, "best_model.pt"))
    ck = torch.load(os.path.join(exp.out_dir, "best_model.pt"), map_location="cpu")
    assert ck["updates"] == 3 and ck["args"]["review_pool"] == 6
    _, again, _ = _run(tmp_path, data_dir, "s1", **kw)
    assert again == losses                                      # same seeds: the same draws, the same steps, bit for bit
    _, other, _ = _run(tmp_path, data_dir, "s2", **dict(kw, review_sample_seed=12))
    assert other != losses                                      # another sampling seed: other reviews
    # counts and pool against the split's rv_num
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    for key, bad in (("u_rv_num", 5), ("i_rv_num", 5), ("review_pool", 3)):
        with pytest.raises(ValueError, match=key):
            ReviewExperiment("simple_siamese", parse_args(_cfg(tmp_path, "simple_siamese", data_dir, "bad", device_reviews=True,
                                                               **dict(kw, **{key: bad}))), uid="bad")


def test_trainer_with_sampling_switched_off_is_the_trainer_without_the_key(tmp_path):
    data_dir = str(tmp_path / "data")
    make_review_dataset.write_review_split(data_dir)
    exp_a, loss_a, log_a = _run(tmp_path, data_dir, "absent")
    exp_f, loss_f, log_f = _run(tmp_path, data_dir, "false", sample_train_review=False)
    assert type(exp_f.train_feed) is type(exp_a.train_feed) and exp_f.cache.pool == exp_a.cache.pool
    assert exp_f.cache.user_pool_table is exp_f.cache.user_table
    assert loss_f == loss_a
    assert "sample_train_review: False" in log_a and "sample_train_review: False" in log_f      # the default is logged either way
    a, f = sorted(log_a), sorted(log_f)                         # the args table lists a given key where the config has it
    assert len(a) == len(f)
    for x, y in zip(a, f):
        if "time: " in x:                                       # the step line ends in the wall time per step
            x, y = x[:x.index("time: ")], y[:y.index("time: ")]
        assert x == y
