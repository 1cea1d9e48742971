"""AHN with the reference's constructor / forward signature, return values and state_dict keys (models/ahn/ahn_model.py:7-92).
The shared BiLSTM sentence encoder -- about nine tenths of the model's arithmetic -- runs on the HIP kernels of
csrc/lstm_seq.hip; the hierarchical co-attention behind it is the torch composition of ahn_layers.py -- or, with `fused_tail`
and in forward_groups (the BPR step: B users against (1 + n_neg) * B items), its user side is one HIP op, forward and backward
(functional.ahn_pair_attend, csrc/ahn_attend.hip)."""
import torch
import torch.nn as nn

from ... import functional as RF
from .ahn_layers import (Embedding, Seq2SeqEncoder, TorchFM, UnbalancedCoAttentionAggregator,
                         UnbalancedCoAttentionAggregatorReview, WordEmbedding)


class AHN(nn.Module):
    def __init__(self, embedding_dim, hidden_dim, k_factor, user_size, item_size, word_vocab_size,
                 pretrained_word_embeddings, rnn_dropout=0., dropout=0.5, item_review_num=None, word_encoder_str="LSTM"):
        super().__init__()
        if word_encoder_str != "LSTM":
            raise ValueError(f"word_encoder_str={word_encoder_str!r}: the HIP encoder covers 'LSTM'")
        if hidden_dim % 2:
            raise ValueError(f"hidden_dim {hidden_dim} must be even (hidden_dim // 2 units per LSTM direction)")
        self.hidden_dim = hidden_dim
        self.word_vocab_size, self.user_size, self.item_size = word_vocab_size, user_size, item_size
        self.validate_ids = True      # device-side range check of every id tensor (functional.sanitize_ids), see DeepCoNNpp
        self.fused_tail = False       # opt-in: aggregate()'s user side on functional.ahn_pair_attend (csrc/ahn_attend.hip)

        self.word_embeddings = WordEmbedding(word_vocab_size, embedding_dim, pretrained_word_embeddings)
        self.word_encoder = Seq2SeqEncoder(nn.LSTM, embedding_dim, hidden_dim // 2, dropout=rnn_dropout, bidirectional=True)
        self.unbalanced_sentence_aggregator = UnbalancedCoAttentionAggregator(hidden_dim, hidden_dim, item_review_num)
        self.user_review_trans_layer = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU())
        self.item_review_trans_layer = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU())
        self.unbalanced_review_aggregator = UnbalancedCoAttentionAggregatorReview(hidden_dim, hidden_dim)
        self.user_embeddings = Embedding(user_size, hidden_dim)
        self.item_embeddigns = Embedding(item_size, hidden_dim)          # the reference's spelling: a state_dict key
        self.dropout = nn.Dropout(p=dropout)
        self.fm = TorchFM(n=hidden_dim * 4, k=k_factor)

    def encode_sentences(self, user_reviews, item_reviews, user_sent_lengths, item_sent_lenghts, drop=None):
        """Word ids [bz, r, s, w] and sentence lengths [bz, r, s] of both sides -> (user_sents [bz, ur, us, hidden],
        item_sents [bz, ir, is, hidden]): lookup, shared BiLSTM, max over the words (ahn_model.py:55-68).  With equal sentence
        widths both sides go through the encoder as ONE batch; each sentence is told its own side's output length, because the
        reference encodes the sides separately and the zero candidate of the max depends on it.  `drop`: the encoder's
        [sentences, E] dropout multiplier drawn by the caller (user rows first) instead of a fresh one."""
        bz, ur_num, us_num, uw_num = user_reviews.shape
        bz_i, ir_num, is_num, iw_num = item_reviews.shape         # forward_groups: B users against G * B items
        table = self.word_embeddings.weight
        pad = self.word_embeddings.padding_idx
        n_u, n_i = bz * ur_num * us_num, bz_i * ir_num * is_num
        u_len = user_sent_lengths.reshape(n_u).to(torch.int64)
        i_len = item_sent_lenghts.reshape(n_i).to(torch.int64)
        t_u, t_i = RF.lstm_t_out(u_len, uw_num), RF.lstm_t_out(i_len, iw_num)
        enc = self.word_encoder
        if uw_num == iw_num:
            ids = torch.cat([user_reviews.reshape(n_u, uw_num), item_reviews.reshape(n_i, iw_num)], dim=0)
            sents = enc.encode_max(RF.embedding(table, ids, pad), torch.cat([u_len, i_len]),
                                   t_out=torch.cat([t_u.expand(n_u), t_i.expand(n_i)]), drop=drop)
            u_sents, i_sents = sents[:n_u], sents[n_u:]
        else:
            u_drop, i_drop = (None, None) if drop is None else (drop[:n_u], drop[n_u:])
            u_sents = enc.encode_max(RF.embedding(table, user_reviews.reshape(n_u, uw_num), pad), u_len, t_out=t_u, drop=u_drop)
            i_sents = enc.encode_max(RF.embedding(table, item_reviews.reshape(n_i, iw_num), pad), i_len, t_out=t_i, drop=i_drop)
        return u_sents.reshape(bz, ur_num, us_num, self.hidden_dim), i_sents.reshape(bz_i, ir_num, is_num, self.hidden_dim)

    def forward_groups(self, user_reviews, item_reviews, user_sent_masks, item_sent_masks, user_sent_lengths, item_sent_lenghts,
                       user_review_masks, item_review_masks, user_ids, item_ids, *, groups):
        """forward()'s ten arguments for G * B rows in the negative sampler's layout (G = `groups` = 1 + n_neg: rows [0, B) the
        observed pairs, rows [(j+1)B, (j+2)B) their j-th negatives, so row g * B + b is user b's) -> forward()'s five outputs for
        the G * B pairs, with every user encoded ONCE: the user side -- reviews, lengths, masks -- is read from the first B rows
        only, the item side from all G * B, and the pair-dependent tail is functional.ahn_pair_attend (one HIP launch forward,
        one backward).  Both sides' sentences go through the encoder as one batch when the word widths agree, each side with its
        own t_out, as in encode_sentences.

        The AHN BPR rule: fed by data.NegativeFeed over a leave-one-out SentenceFeed, a user is represented -- for the observed
        item AND for its negatives -- by the observed pair's leave-one-out reviews.  This is a definition, not what forward() on
        the expanded batch computes: there a negative's own user rows are gathered for the pair (u, i-), which has no review
        to leave out, i.e. the plain first rv_num reviews.  forward_groups equals forward() on the expanded batch whose user
        rows are the first B rows repeated G times.  Everything but the encoder and the tail is the torch composition of
        aggregate()."""
        G = int(groups)
        P = item_reviews.shape[0]
        if G < 1 or P % G or user_reviews.shape[0] != P:
            raise ValueError(f"forward_groups: {P} item rows / {user_reviews.shape[0]} user rows are not groups={groups} x B pairs")
        B = P // G
        if self.validate_ids:
            user_reviews, item_reviews, user_ids, item_ids = RF.sanitize_ids(
                [(user_reviews, self.word_vocab_size, 0), (item_reviews, self.word_vocab_size, 0), (user_ids, self.user_size, 0),
                 (item_ids, self.item_size, 0)])
        user_sents, item_sents = self.encode_sentences(user_reviews[:B], item_reviews, user_sent_lengths[:B], item_sent_lenghts)
        return self._aggregate_fused(user_sents, item_sents, user_sent_masks[:B], item_sent_masks, user_review_masks[:B],
                                     item_review_masks, user_ids, item_ids, G)

    def forward(self, user_reviews, item_reviews, user_sent_masks, item_sent_masks, user_sent_lengths, item_sent_lenghts,
                user_review_masks, item_review_masks, user_ids, item_ids):
        """user_reviews [bz, ur_num, us_num, uw_num] / item_reviews [bz, ir_num, is_num, iw_num] int64 word ids, sentence masks
        and lengths [bz, r_num, s_num], review masks [bz, r_num], ids [bz] -> (out_logits [bz], user_sent_weights
        [bz, ur_num, us_num], item_sent_weights [bz, ir_num, is_num], user_review_weights [bz, ur_num], item_review_weights
        [bz, ir_num])."""
        if self.validate_ids:
            user_reviews, item_reviews, user_ids, item_ids = RF.sanitize_ids(
                [(user_reviews, self.word_vocab_size, 0), (item_reviews, self.word_vocab_size, 0), (user_ids, self.user_size, 0),
                 (item_ids, self.item_size, 0)])
        user_sents, item_sents = self.encode_sentences(user_reviews, item_reviews, user_sent_lengths, item_sent_lenghts)
        return self.aggregate(user_sents, item_sents, user_sent_masks, item_sent_masks, user_review_masks, item_review_masks,
                              user_ids, item_ids)

    # ------------------------------------------------------------------ per-id sentence tables (recommend.AhnRecommender)
    # The co-attention is asymmetric: the item side is pooled by GatedAttention alone, only the user side looks at the pair, and
    # the encoder -- nine tenths of the arithmetic -- depends on the id only.  encode_users / encode_items cut the eval-mode
    # forward at that line; functional.ahn_pair_score (csrc/ahn_pair.hip) is the rest.  A cached sentence vector needs a FIXED
    # t_out (the zero candidate of the max over the words depends on the batch's longest sentence): the caller
    # passes, per side, one device int32 -- AhnRecommender takes the longest clamped sentence of the whole table -- and a table
    # score equals forward() on a batch whose longest sentence per side is that value.
    def _encode_side(self, reviews, sent_lens, t_out):
        n, r_num, s_num, w_num = reviews.shape
        rows = RF.embedding(self.word_embeddings.weight, reviews.reshape(n * r_num * s_num, w_num), self.word_embeddings.padding_idx)
        return self.word_encoder.encode_max(rows, sent_lens.reshape(-1).to(torch.int64), t_out=t_out).view(n, r_num, s_num, self.hidden_dim)

    def word_contributions(self, user_reviews, item_reviews, user_sent_masks, item_sent_masks, user_sent_lengths, item_sent_lenghts,
                           user_review_masks, item_review_masks, user_ids, item_ids, t_out_user, t_out_item):
        """forward()'s ten arguments for n pairs plus each side's fixed output length (device int32 [1], as _encode_side takes it)
        -> (score [n], user_words [n, Ru, Su, W, 2], item_words [n, Ri, Si, W, 2], user_sentences [n, Ru, Su], item_sentences
        [n, Ri, Si], user_sents [n, Ru, Su, F], item_sents [n, Ri, Si, F]); eval semantics.

        Both sides' sentences are re-encoded with the encoder's state kept (functional.bilstm_encode_states; one batch when the
        word widths agree, each sentence with its own side's t_out, as in encode_sentences), aggregate() runs under autograd on
        the DETACHED sentence vectors, pair by pair, and each score is differentiated for d score / d sentence vector of both
        sides -- the item's through its match AND its own GatedAttention path -- and functional.lstm_seq_word_saliency takes each
        gradient down to the words: *_words[..., w, d] = <d score / d x_w, x_w> through direction d of the BiLSTM, x_w the
        word's embedding.  *_sentences = <d score / d sentence vector, sentence vector>."""
        n, ur_num, us_num, uw_num = user_reviews.shape
        _, ir_num, is_num, iw_num = item_reviews.shape
        n_u, n_i = n * ur_num * us_num, n * ir_num * is_num
        F_ = self.hidden_dim
        table, pad = self.word_embeddings.weight, self.word_embeddings.padding_idx
        u_len, i_len = user_sent_lengths.reshape(n_u).to(torch.int64), item_sent_lenghts.reshape(n_i).to(torch.int64)
        params = self.word_encoder.lstm_params()
        with RF.eval_mode(self):
            if uw_num == iw_num:
                sides = [(torch.cat([user_reviews.reshape(n_u, uw_num), item_reviews.reshape(n_i, iw_num)], dim=0),
                          torch.cat([u_len, i_len]), torch.cat([t_out_user.expand(n_u), t_out_item.expand(n_i)]))]
            else:
                sides = [(user_reviews.reshape(n_u, uw_num), u_len, t_out_user), (item_reviews.reshape(n_i, iw_num), i_len, t_out_item)]
            enc = [RF.bilstm_encode_states(RF.embedding(table, ids, pad), params, lens, t_out=t_out) for ids, lens, t_out in sides]
            pooled = torch.cat([e[1] for e in enc], dim=0)
            xu, xi = pooled[:n_u].view(n, ur_num, us_num, F_), pooled[n_u:].view(n, ir_num, is_num, F_)
            score, gu, gi = [], [], []
            with torch.enable_grad():
                # one pair at a time: torch picks its product kernels by the batch's size, and a pair's bits must not depend on
                # the pairs explained beside it (the tail is a few hundred rows; the encoder above is the arithmetic)
                for b in range(n):
                    s = slice(b, b + 1)
                    xu_b, xi_b = xu[s].detach().requires_grad_(True), xi[s].detach().requires_grad_(True)
                    sc = self.aggregate(xu_b, xi_b, user_sent_masks[s], item_sent_masks[s], user_review_masks[s],
                                        item_review_masks[s], user_ids[s], item_ids[s])[0]
                    g = torch.autograd.grad(sc.sum(), (xu_b, xi_b))
                    score.append(sc.detach())
                    gu.append(g[0])
                    gi.append(g[1])
            score, gu, gi = torch.cat(score), torch.cat(gu), torch.cat(gi)
            d_pooled = torch.cat([gu.reshape(n_u, F_), gi.reshape(n_i, F_)], dim=0)
            words, a = [], 0
            for (_, lens, _), (xw, _, argmax, state) in zip(sides, enc):
                words.append(RF.lstm_seq_word_saliency(state, xw, params[1], params[5], lens, d_pooled[a:a + state.N], argmax))
                a += state.N
            words = [words[0][:n_u], words[0][n_u:]] if len(words) == 1 else words
            return (score, words[0].reshape(n, ur_num, us_num, uw_num, 2), words[1].reshape(n, ir_num, is_num, iw_num, 2),
                    (gu * xu).sum(-1), (gi * xi).sum(-1), xu, xi)

    def _fm_blocks(self):
        """fm.V and fm.lin.weight cut into the four blocks of final_features = [z, e_u, q, e_i]."""
        F_ = self.hidden_dim
        V, lw = self.fm.V.detach(), self.fm.lin.weight.detach().view(-1)
        return [V[b * F_:(b + 1) * F_] for b in range(4)], [lw[b * F_:(b + 1) * F_] for b in range(4)]

    @staticmethod
    def _fm_partial(x, V, lw):
        """[n, K + 2] of the rows x [n, F]: x V, sum_k (x^2 V^2)_k, x . lw -- a block's share of TorchFM.forward."""
        return torch.cat([x @ V, ((x * x) @ (V * V)).sum(1, keepdim=True), (x @ lw).unsqueeze(1)], dim=1)

    def user_state(self, user_sents, sent_masks, rev_masks, ids) -> "RF.AhnUserState":
        """encode_users behind the encoder: sentence vectors [n, Ru, Su, F] -> the state rows."""
        n, r_num, s_num, F_ = user_sents.shape
        with RF.eval_mode(self):
            X = user_sents.detach().reshape(n * r_num * s_num, F_).contiguous()
            Xt = RF.linear(X, self.user_review_trans_layer[0].weight.detach())
            Vb, lb = self._fm_blocks()
            fm = self._fm_partial(self.user_embeddings(ids), Vb[1], lb[1])
        return RF.AhnUserState(X.view(n, r_num * s_num, F_), Xt.view(n, r_num * s_num, F_), sent_masks.bool(), rev_masks.bool(), fm)

    def item_state(self, item_sents, sent_masks, rev_masks, ids) -> "RF.AhnItemState":
        """encode_items behind the encoder: sentence vectors [n, Ri, Si, F] -> the state rows, from the existing modules."""
        n, r_num, s_num, F_ = item_sents.shape
        sa, ra = self.unbalanced_sentence_aggregator, self.unbalanced_review_aggregator
        with RF.eval_mode(self):
            Y = item_sents.detach().reshape(n * r_num, s_num, F_)
            r, sent_w, all_w = sa.item_aggregator(Y, sent_masks.reshape(n * r_num, s_num).bool())
            Ks = RF.linear((all_w.reshape(n * r_num * s_num, 1) * Y.reshape(n * r_num * s_num, F_)).contiguous(), sa.bilinear.weight.detach())
            r = self.item_review_trans_layer(r)
            q, rev_w = ra.item_aggregator(r, rev_masks.bool())
            Kr = RF.linear(r.reshape(n * r_num, F_).contiguous(), ra.bilinear.weight.detach())
            Vb, lb = self._fm_blocks()
            fm = self._fm_partial(q, Vb[2], lb[2]) + self._fm_partial(self.item_embeddigns(ids), Vb[3], lb[3])
        return RF.AhnItemState(Ks.view(n, r_num * s_num, F_), Kr.view(n, r_num, F_), fm, sent_w, rev_w)

    def item_reviews(self, item_sents, sent_masks) -> torch.Tensor:
        """The transformed item reviews r' [n, Ri, F] of the sentence vectors [n, Ri, Si, F] item_state is given: what its Kr
        (= r' @ Wr^T) and the pooled item q (= sum_i item_review_weights[i] r'[i]) are made of, by the same modules.  The item's
        own path into the FM, for functional.ahn_pair_explain."""
        n, r_num, s_num, F_ = item_sents.shape
        with RF.eval_mode(self):
            r, _, _ = self.unbalanced_sentence_aggregator.item_aggregator(item_sents.detach().reshape(n * r_num, s_num, F_),
                                                                          sent_masks.reshape(n * r_num, s_num).bool())
            return self.item_review_trans_layer(r).detach().view(n, r_num, F_)

    def encode_users(self, reviews, sent_masks, sent_lens, rev_masks, ids, t_out) -> "RF.AhnUserState":
        """Word ids [n, Ru, Su, W], sentence masks / lengths [n, Ru, Su], review masks [n, Ru], user ids [n] and the side's fixed
        output length t_out (device int32 [1], functional.lstm_t_out) -> the per-user state of the pair tail; eval semantics."""
        with RF.eval_mode(self):
            sents = self._encode_side(reviews, sent_lens, t_out)
        return self.user_state(sents, sent_masks, rev_masks, ids)

    def encode_items(self, reviews, sent_masks, sent_lens, rev_masks, ids, t_out) -> "RF.AhnItemState":
        """The item side of encode_users; the state carries item_sent_weights [n, Ri, Si] and item_review_weights [n, Ri], which
        no pair changes."""
        with RF.eval_mode(self):
            sents = self._encode_side(reviews, sent_lens, t_out)
        return self.item_state(sents, sent_masks, rev_masks, ids)

    def pair_head(self) -> "RF.AhnPairHead":
        """What the pair tail reads of the parameters: user_review_trans_layer's bias and the FM's z block (its per-id blocks are
        in the states' fm rows).  A snapshot, like the tables."""
        Vb, lb = self._fm_blocks()
        return RF.AhnPairHead(self.user_review_trans_layer[0].bias.detach().clone(), Vb[0].t().contiguous(),
                              (Vb[0] * Vb[0]).sum(1).contiguous(), lb[0].contiguous().clone(), self.fm.lin.bias.detach().clone())

    def explain_head(self):
        """(VqT [K, F], vq2 [F], lq [F]): the FM's block of the item's pooled vector q, cut as pair_head cuts z's block.  A
        snapshot, like the tables; with AHN.item_reviews the rest of functional.AhnExplainRows."""
        Vb, lb = self._fm_blocks()
        return Vb[2].t().contiguous(), (Vb[2] * Vb[2]).sum(1).contiguous(), lb[2].contiguous().clone()

    def aggregate(self, user_sents, item_sents, user_sent_masks, item_sent_masks, user_review_masks, item_review_masks,
                  user_ids, item_ids):
        """Everything behind the sentence vectors (ahn_model.py:70-92): the torch composition, on the inputs' device; with
        `fused_tail` the user side runs on functional.ahn_pair_attend instead (_aggregate_fused at one group)."""
        if self.fused_tail:
            return self._aggregate_fused(user_sents, item_sents, user_sent_masks, item_sent_masks, user_review_masks,
                                         item_review_masks, user_ids, item_ids, 1)
        user_reviews, item_reviews, user_sent_weights, item_sent_weights, _ = self.unbalanced_sentence_aggregator(
            user_sents, item_sents, user_sent_masks, item_sent_masks)
        user_reviews = self.user_review_trans_layer(user_reviews)
        item_reviews = self.item_review_trans_layer(item_reviews)
        rv_users, rv_items, user_review_weights, item_review_weights = self.unbalanced_review_aggregator(
            user_reviews, item_reviews, user_review_masks, item_review_masks)
        users = torch.cat([rv_users, self.user_embeddings(user_ids)], dim=-1)
        items = torch.cat([rv_items, self.item_embeddigns(item_ids)], dim=-1)
        final_features = self.dropout(torch.cat([users, items], dim=-1))
        out_logits = self.fm(final_features).view(-1)
        return out_logits, user_sent_weights, item_sent_weights, user_review_weights, item_review_weights

    def _aggregate_fused(self, user_sents, item_sents, user_sent_masks, item_sent_masks, user_review_masks, item_review_masks,
                         user_ids, item_ids, groups):
        """aggregate() for B users [B, Ru, Su, F] against groups * B items [G * B, Ri, Si, F] (pair g * B + b is user b's), with
        the user side's co-attention on functional.ahn_pair_attend (csrc/ahn_attend.hip, forward and backward).  The op takes the
        three products of the user side's parameters as inputs -- Xt = X Wt^T, Ks = (a * Y) Ws^T, Kr = r' Wr^T, each the
        autograd `linear` -- which moves user_review_trans_layer's product in front of the weighted sum: a reassociation of
        aggregate()'s arithmetic, not its bits.  The item side (GatedAttention, item_review_trans_layer), the id embeddings, the
        dropout and the FM are aggregate()'s torch composition."""
        sa, ra = self.unbalanced_sentence_aggregator, self.unbalanced_review_aggregator
        n_u, ur_num, us_num, F_ = user_sents.shape
        n_i, ir_num, is_num, _ = item_sents.shape
        item_rows = item_sents.reshape(n_i * ir_num, is_num, F_)
        item_reviews, item_sent_weights, item_all_sent_weights = sa.item_aggregator(
            item_rows, item_sent_masks.reshape(n_i * ir_num, is_num))
        Ks = RF.linear((item_all_sent_weights.reshape(n_i * ir_num * is_num, 1) * item_rows.reshape(n_i * ir_num * is_num, F_)).contiguous(),
                       sa.bilinear.weight)
        item_reviews = self.item_review_trans_layer(item_reviews)
        rv_items, item_review_weights = ra.item_aggregator(item_reviews, item_review_masks)
        Kr = RF.linear(item_reviews.reshape(n_i * ir_num, F_).contiguous(), ra.bilinear.weight)
        trans = self.user_review_trans_layer[0]
        X = user_sents.reshape(n_u * ur_num * us_num, F_).contiguous()
        Xt = RF.linear(X, trans.weight)
        rv_users, user_sent_weights, user_review_weights = RF.ahn_pair_attend(
            X.view(n_u, ur_num * us_num, F_), Xt.view(n_u, ur_num * us_num, F_), user_sent_masks, user_review_masks,
            Ks.view(n_i, ir_num * is_num, F_), Kr.view(n_i, ir_num, F_), trans.bias, groups=groups)
        users = torch.cat([rv_users, self.user_embeddings(user_ids)], dim=-1)
        items = torch.cat([rv_items, self.item_embeddigns(item_ids)], dim=-1)
        final_features = self.dropout(torch.cat([users, items], dim=-1))
        out_logits = self.fm(final_features).view(-1)
        return out_logits, user_sent_weights, item_sent_weights, user_review_weights, item_review_weights
