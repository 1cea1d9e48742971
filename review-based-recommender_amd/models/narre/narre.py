"""NARRE with the reference's constructor / forward signature and state_dict keys
(models/narre/narre.py:139-192), running on the HIP kernels of csrc/.

narre.py defines its OWN WordEmbedding / LinearAttention / LastFeat / FM (narre.py:9-137), with
b = g_bias = 0.1 initialisation; those are mirrored here (the LastFeat / FM mirrors of
models/deepconn/layers.py initialise identically, so they are shared)."""
import torch
import torch.nn as nn

from ... import functional as RF
from ..deepconn.layers import FM, LastFeat, WordEmbedding, latent_rows, rating_head
from .layers import NgramFeat


class LinearAttention(nn.Module):
    """narre.py:26-64: review-level attention conditioned on the counterpart-id embedding.
    att = exp(logit) / (sum_R exp(logit) + 1e-8): un-masked, no max subtraction (quirk 3)."""

    def __init__(self, vocab_size, feat_size, hidden_dim, dropout, padding_idx=0):
        super().__init__()
        self.padding_idx = padding_idx
        self.W_rv = nn.Parameter(torch.empty(feat_size, hidden_dim).uniform_(-0.1, 0.1))
        self.W_id = nn.Parameter(torch.empty(hidden_dim, hidden_dim).uniform_(-0.1, 0.1))
        self.h = nn.Parameter(torch.empty(hidden_dim, 1).uniform_(-0.1, 0.1))
        self.b_1 = nn.Parameter(torch.empty(hidden_dim).fill_(0.1))
        self.b_2 = nn.Parameter(torch.empty(1).fill_(0.1))
        self.ebd_vals = nn.Embedding(vocab_size, hidden_dim, padding_idx=padding_idx)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, feat, other_id):
        """feat [bz, dnum, hidden], other_id [bz, dnum] -> (out [bz, hidden], att_scores [bz, dnum, 1])."""
        drop = RF.dropout_multiplier((feat.shape[0], feat.shape[2]), self.dropout.p, self.training, feat.device)
        return RF.review_attention(feat, other_id, self.W_rv, self.W_id, self.h, self.b_1, self.b_2,
                                   self.ebd_vals.weight, pad_idx=self.padding_idx, drop=drop)


class NARRE(nn.Module):
    def __init__(self, user_size, item_size, vocab_size, kernel_sizes, hidden_dim, embedding_dim, att_dim, latent_dim,
                 max_doc_num, max_doc_len, dropout, word_padding_idx, user_padding_idx, item_padding_idx,
                 pretrained_embeddings, arch):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.hiddem_dim = hidden_dim      # (sic) attribute name of the reference
        self.doc_num = max_doc_num
        self.doc_len = max_doc_len

        # narre.py:151 does not forward word_padding_idx to WordEmbedding: padding_idx stays 0
        self.word_embeddings = WordEmbedding(vocab_size, embedding_dim, pretrained_embeddings=pretrained_embeddings)
        self.ngram = NgramFeat(kernel_sizes, embedding_dim, hidden_dim, max_doc_len, arch=arch)
        self.user_att = LinearAttention(item_size, hidden_dim, att_dim, dropout, padding_idx=item_padding_idx)
        self.item_att = LinearAttention(user_size, hidden_dim, att_dim, dropout, padding_idx=user_padding_idx)
        self.user_feat = LastFeat(user_size, hidden_dim, latent_dim, padding_idx=user_padding_idx)
        self.item_feat = LastFeat(item_size, hidden_dim, latent_dim, padding_idx=item_padding_idx)
        self.fm = FM(user_size, item_size, latent_dim, dropout, user_padding_idx=user_padding_idx,
                     item_padding_idx=item_padding_idx)
        self.user_size, self.item_size, self.vocab_size = user_size, item_size, vocab_size
        self.validate_ids = True      # device-side range check of every id tensor (functional.sanitize_ids), see DeepCoNNpp

    def forward(self, u_text, i_text, u_text_masks, i_text_masks, u_id, i_id, reuid, reiid):
        """u_text/i_text [bz, doc_num, doc_len] int64, masks same shape bool, u_id/i_id [bz],
        reuid/reiid [bz, doc_num]  ->  (pred [bz], u_att [bz, doc_num, 1], i_att [bz, doc_num, 1]).

        Reviews are folded into the batch (narre.py:170-176); both sides go through ONE launch of the
        fused gather+conv+pool kernel as 2*bz*doc_num documents of doc_len tokens."""
        bz = u_text.shape[0]
        R, T = self.doc_num, self.doc_len
        if self.validate_ids:
            wp = self.word_embeddings.padding_idx
            ids, u_id, i_id, reuid, reiid = RF.sanitize_ids(
                [(u_text.reshape(-1, T), self.vocab_size, wp), (i_text.reshape(-1, T), self.vocab_size, wp),
                 (u_id, self.user_size, self.user_feat.padding_idx), (i_id, self.item_size, self.item_feat.padding_idx),
                 (reuid, self.item_size, self.user_att.padding_idx), (reiid, self.user_size, self.item_att.padding_idx)],
                stack_first_two=True)
        else:
            ids = RF.stack_rows(u_text.reshape(-1, T), i_text.reshape(-1, T))
        masks = RF.stack_rows(u_text_masks.reshape(-1, T), i_text_masks.reshape(-1, T))
        feats = self.ngram.encode(self.word_embeddings.weight, ids, masks, padding_idx=self.word_embeddings.padding_idx)
        # both attention pools (user_att keyed by item ids, item_att by user ids: narre.py:177-178) in ONE launch per stage: the conv
        # output is already the stacked [2, bz, R, H] block, the pooled features go to the rating head as one [2*bz, H] block, and
        # so do the gradients on the way back -- no unbind / stack, no second stream
        ua, ia = self.user_att, self.item_att
        other = RF.stack_rows(reuid, reiid).view(2, bz, R)          # a view when the two id tensors are neighbours (sanitize_ids, the step's input block)
        drop = RF.dropout_multiplier((2 * bz, self.hiddem_dim), ua.dropout.p, ua.training, feats.device)
        out, att = RF.review_attention2(
            feats.view(2, bz, R, self.hiddem_dim), other,
            (ua.W_rv, ua.W_id, ua.h, ua.b_1, ua.b_2, ua.ebd_vals.weight), (ia.W_rv, ia.W_id, ia.h, ia.b_1, ia.b_2, ia.ebd_vals.weight),
            pad_idx=(ua.padding_idx, ia.padding_idx), drop=None if drop is None else drop.view(2, bz, self.hiddem_dim))
        u_att_scores, i_att_scores = att[0], att[1]

        pred = rating_head(self.user_feat, self.item_feat, self.fm, out.view(2 * bz, self.hiddem_dim), None, u_id, i_id)
        return pred.view(-1), u_att_scores, i_att_scores

    def pair_latents(self, u_text, i_text, u_text_masks, i_text_masks, u_id, i_id, reuid, reiid):
        """forward's arguments -> (ul, il) [bz, latent_dim] each: the towers' latent rows, under autograd and in the module's own
        train / eval mode (the attention pools keep their dropout).  Encoder and both attention pools run once on the stacked
        batch, as in forward; the tail stops at LastFeat, so that a loss over all bz x bz pairs of the batch
        (functional.pair_softmax_loss) can follow.  forward is untouched."""
        bz = u_text.shape[0]
        R, T = self.doc_num, self.doc_len
        if self.validate_ids:
            wp = self.word_embeddings.padding_idx
            ids, u_id, i_id, reuid, reiid = RF.sanitize_ids(
                [(u_text.reshape(-1, T), self.vocab_size, wp), (i_text.reshape(-1, T), self.vocab_size, wp),
                 (u_id, self.user_size, self.user_feat.padding_idx), (i_id, self.item_size, self.item_feat.padding_idx),
                 (reuid, self.item_size, self.user_att.padding_idx), (reiid, self.user_size, self.item_att.padding_idx)],
                stack_first_two=True)
        else:
            ids = RF.stack_rows(u_text.reshape(-1, T), i_text.reshape(-1, T))
        masks = RF.stack_rows(u_text_masks.reshape(-1, T), i_text_masks.reshape(-1, T))
        feats = self.ngram.encode(self.word_embeddings.weight, ids, masks, padding_idx=self.word_embeddings.padding_idx)
        ua, ia = self.user_att, self.item_att
        other = RF.stack_rows(reuid, reiid).view(2, bz, R)
        drop = RF.dropout_multiplier((2 * bz, self.hiddem_dim), ua.dropout.p, ua.training, feats.device)
        out, _ = RF.review_attention2(
            feats.view(2, bz, R, self.hiddem_dim), other,
            (ua.W_rv, ua.W_id, ua.h, ua.b_1, ua.b_2, ua.ebd_vals.weight), (ia.W_rv, ia.W_id, ia.h, ia.b_1, ia.b_2, ia.ebd_vals.weight),
            pad_idx=(ua.padding_idx, ia.padding_idx), drop=None if drop is None else drop.view(2, bz, self.hiddem_dim))
        return latent_rows(self.user_feat, self.item_feat, out.view(2 * bz, self.hiddem_dim), u_id, i_id)

    # ---- one tower at a time (recommend.Recommender).  The attention pool of a side is keyed by its reviews' own counterpart
    # ids (reuid / reiid, narre.py:177-178), not by the target pair, so a side's latent row is a function of that side alone.
    def _encode_side(self, text, masks, my_id, other_id, my_rows, other_rows, att, last):
        with RF.eval_mode(self):
            n, T = text.shape[0], self.doc_len
            wp = self.word_embeddings.padding_idx
            text, masks = text.reshape(-1, T), masks.reshape(-1, T)
            if self.validate_ids:
                text, other_id = RF.sanitize_ids([(text, self.vocab_size, wp), (other_id, other_rows, att.padding_idx)])
            feats = self.ngram.encode(self.word_embeddings.weight, text.contiguous(), masks.contiguous(), padding_idx=wp)
            pooled, _ = att(feats.view(n, self.doc_num, self.hiddem_dim), other_id)
            return last(pooled, my_id)         # LastFeat checks its ids itself

    def encode_users(self, u_text, u_text_masks, u_id, reuid):
        """u_text / masks [n, doc_num, doc_len], u_id [n], reuid [n, doc_num] (item ids of the user's reviews) -> the users' latent
        rows [n, latent_dim] in eval semantics, no autograd.  Any n: the item side is not needed."""
        return self._encode_side(u_text, u_text_masks, u_id, reuid, self.user_size, self.item_size, self.user_att, self.user_feat)

    def encode_items(self, i_text, i_text_masks, i_id, reiid):
        """The item tower's counterpart of encode_users (reiid: user ids of the item's reviews)."""
        return self._encode_side(i_text, i_text_masks, i_id, reiid, self.item_size, self.user_size, self.item_att, self.item_feat)

    # ---- why a pair scored as it did: per-review and per-token contributions of one tower (recommend.Recommender.explain)
    def _explain_side(self, text, masks, other_id, other_rows, att, last, d_latent):
        if self.ngram.arch != "CNN":
            raise ValueError("explain_users / explain_items cover DeepCoNN++ and NARRE with arch='CNN' (the TextCNN's max-pool "
                             f"routing is what they read); arch={self.ngram.arch!r} is not covered")
        with RF.eval_mode(self):
            n, R, T, H = text.shape[0], self.doc_num, self.doc_len, self.hiddem_dim
            wp = self.word_embeddings.padding_idx
            text, masks = text.reshape(-1, T), masks.reshape(-1, T)
            if self.validate_ids:
                text, other_id = RF.sanitize_ids([(text, self.vocab_size, wp), (other_id, other_rows, att.padding_idx)])
            conv, table = self.ngram.feature_layer[0], self.word_embeddings.weight
            text, masks = text.contiguous(), masks.contiguous()
            feat, argmax = RF.textcnn(table, text, masks, conv.weights(), conv.biases(), padding_idx=wp, return_argmax=True)
            _, a = att(feat.view(n, R, H), other_id)
            a = a.view(n, R)
            g = RF.linear(d_latent, last.W)                                   # d score / d pooled = d_latent @ W^T  [n, H]
            reviews = a * (g.unsqueeze(1) * feat.view(n, R, H)).sum(-1)
            d_feat = (a.unsqueeze(-1) * g.unsqueeze(1)).reshape(n * R, H)      # attention weights held constant
            tokens = RF.textcnn_saliency(table, text, masks, conv.weights(), feat, argmax, d_feat).view(n, R, T)
            return tokens, reviews.sum(1), a, reviews

    def explain_users(self, u_text, u_text_masks, u_id, reuid, d_latent):
        """encode_users' arguments plus d_latent [n, latent_dim] = d score / d (the users' latent rows) -> (tokens [n, doc_num,
        doc_len], text [n], att [n, doc_num], reviews [n, doc_num]) in eval semantics, no autograd.
        The attention weights att are HELD CONSTANT -- the NARRE paper's reading of att as the usefulness of a review: with
        g = d score / d (pooled feature), review r contributes reviews[n, r] = att[n, r] * <g, feat[n, r]>, text = reviews.sum(1),
        and tokens[n, r, t] is gradient x input of the token's embedded row under the gradient att[n, r] * g on the review's
        pooled features, max-pool routing fixed (functional.textcnn_saliency).  How the score would move through a change of
        att itself is not attributed.  CNN arch only."""
        return self._explain_side(u_text, u_text_masks, reuid, self.item_size, self.user_att, self.user_feat, d_latent)

    def explain_items(self, i_text, i_text_masks, i_id, reiid, d_latent):
        """The item tower's counterpart of explain_users (reiid: user ids of the item's reviews)."""
        return self._explain_side(i_text, i_text_masks, reiid, self.user_size, self.item_att, self.item_feat, d_latent)

    def score_mode_and_params(self):
        """(mode, h, g, ub, ib) of functional.pair_score*: the FM head over the two latent rows (narre.py:112-137)."""
        fm = self.fm
        return "fm", fm.h, fm.g_bias, fm.user_bias.weight, fm.item_bias.weight
