"""D-ATT (dual local/global attention) with the reference's constructor / forward signature and
state_dict keys (models/dual_att/dual_att.py:19-61), running on the HIP kernels of csrc/.

The reference file's legacy `__main__` block (dual_att.py:63-150; undefined ReviewData / CNNDLGA) and its
unused nltk / pandas imports are not part of the model and have no counterpart here."""
import os

import torch
import torch.nn as nn

from ... import functional as RF
from .layers import GlobalAttention, LocalAttention, WordEmbedding


class DualAtt(nn.Module):
    def __init__(self, vocab_size, doc_len, l_window_size=5, l_out_size=200, g_out_size=100, emb_size=100,
                 hidden_size_1=500, hidden_size_2=50, dropout=0.5, pretrained_embeddings=None):
        super().__init__()
        self.fc_input = l_out_size + 3 * g_out_size
        self.vocab_size = vocab_size
        self.validate_ids = True      # device-side range check of the token ids (functional.sanitize_ids), see DeepCoNNpp

        self.word_embeddings = WordEmbedding(vocab_size, emb_size, pretrained_embeddings=pretrained_embeddings)
        self.u_local_atten = LocalAttention(doc_len, l_window_size, l_out_size, emb_size)
        self.u_global_atten = GlobalAttention(doc_len, g_out_size, emb_size)
        self.i_local_atten = LocalAttention(doc_len, l_window_size, l_out_size, emb_size)
        self.i_global_atten = GlobalAttention(doc_len, g_out_size, emb_size)
        # ONE fc shared by both towers (dual_att.py:31,51,57); kept as nn.Sequential for the state_dict keys fc.0 / fc.3
        self.fc = nn.Sequential(nn.Linear(self.fc_input, hidden_size_1), nn.ReLU(), nn.Dropout(dropout),
                                nn.Linear(hidden_size_1, hidden_size_2))

    @staticmethod
    def _merged_applies(local, table, docs, weights, pad):
        """True when the tower's two gated convs run as ONE conv call of four banks under a split gate (_encode)."""
        return (local.conv[0].kernel_size[0] == 1 and os.environ.get("RBR_DATT_MERGED", "1") != "0"
                and RF.textcnn_product_applies(table, docs, weights, RF.PAD_VALID, RF.ACT_TANH, pad))

    def _encode(self, docs, local, glob, tabs):
        """`tabs`: four aliases of the word table (RF.table_fanout), one per table-consuming op of the tower."""
        pad = self.word_embeddings.padding_idx
        rows = RF.datt_token_rows(docs, tabs[0].shape[0])      # distinct-token maps, once per tower: both gates work on them
        convs = [local.conv[0], glob.conv1[0], glob.conv2[0], glob.conv3[0]]
        weights = [c.weight for c in convs]
        if self._merged_applies(local, tabs[1], docs, weights, pad):
            # The tower's two gated convs read the same tokens: as ONE conv call of four banks -- the 1-wide local conv ('same'
            # = 'valid' at width 1) under the local gate, the 2/3/4-wide global convs under the global gate
            # (RBR_CONV_GATE_SPLIT) -- they share the token list, the product-table GEMM, the gather launch, and in the
            # backward G and the sparse product.  Same results (layers.py:43-53,81-89); channels come back local first.
            gate_l = RF.datt_gate(tabs[0], local.attn[0].weight, local.attn[0].bias, docs, is_global=False, padding_idx=pad,
                                  rows=rows)
            gate_g = RF.datt_gate(tabs[2], glob.attn[0].weight, glob.attn[0].bias, docs, is_global=True, padding_idx=pad,
                                  rows=rows)
            feat = RF.textcnn(tabs[1], docs, None, weights, [c.bias for c in convs], gate=(gate_l, gate_g), gate_split=1,
                              pad_mode=RF.PAD_VALID, act=RF.ACT_TANH, padding_idx=pad, pad_runs=local.window_size <= 17)
            return feat, None                                   # [bz, l_out + 3 * g_out]: cat((local, global), 1) already
        return local.encode(tabs[0:2], docs, pad, rows=rows), glob.encode(tabs[2:4], docs, pad, rows=rows)

    def _fc(self, feat):
        p = self.fc[2].p
        drop = RF.dropout_multiplier((feat.shape[0], self.fc[0].out_features), p, self.training, feat.device)
        hid = RF.linear(feat, self.fc[0].weight, self.fc[0].bias, relu=True, drop=drop)
        return RF.linear(hid, self.fc[3].weight, self.fc[3].bias)

    def _tower_params(self, local, glob):
        convs = [local.conv[0], glob.conv1[0], glob.conv2[0], glob.conv3[0]]
        return (local.attn[0].weight, local.attn[0].bias, glob.attn[0].weight, glob.attn[0].bias,
                [c.weight for c in convs], [c.bias for c in convs])

    def forward(self, u_docs, i_docs):
        """u_docs / i_docs [bz, doc_len] int64 -> ratings [bz]."""
        bz = u_docs.shape[0]
        pad = self.word_embeddings.padding_idx
        if self.validate_ids:
            u_docs, i_docs = RF.sanitize_ids([(u_docs, self.vocab_size, pad), (i_docs, self.vocab_size, pad)])
        # Both towers through every kernel in ONE pass (RF.datt_towers): the towers run the same ops on separate parameters and
        # documents of equal shapes (dual_att.py:45-57), so each kernel of the chain -- token rows, both gates, the merged
        # four-bank conv, and their backwards -- is launched once with gridDim.z = 2 instead of once per tower.
        u_par, i_par = self._tower_params(self.u_local_atten, self.u_global_atten), self._tower_params(self.i_local_atten, self.i_global_atten)
        if u_docs.shape == i_docs.shape and self.u_local_atten.window_size == self.i_local_atten.window_size:
            docs2 = RF.stack_rows(u_docs, i_docs)
            if RF.datt_pair_applies(self.word_embeddings.weight, docs2, u_par[0], u_par[4]):
                feats = RF.datt_towers(self.word_embeddings.weight, docs2, u_par, i_par, padding_idx=pad,
                                       pad_runs=self.u_local_atten.window_size <= 17)
                return RF.pair_dot(self._fc(feats)).view(-1)                # sum(u_feat * i_feat, 1)  (dual_att.py:58)
        # eight ops of the step produce gradient for the word table (a gate and a conv, local and global, per tower): each gets
        # its own alias, and their backwards add their rows into one buffer instead of eight dense gradients summed by autograd
        # (Tried in round 3 and dropped: the item tower on a stream of its own, so that one tower's ~40 latency-bound launches run
        # under the other's long kernels -- autograd then replays every backward op on its forward's stream, and recording that
        # backward into a hipGraph crashed the process inside the capture; the towers stay one after the other.)
        tabs = RF.table_fanout(self.word_embeddings.weight, 8)
        u_loc, u_glo = self._encode(u_docs, self.u_local_atten, self.u_global_atten, tabs[0:4])
        i_loc, i_glo = self._encode(i_docs, self.i_local_atten, self.i_global_atten, tabs[4:8])
        # the fc is ONE module shared by both towers (dual_att.py:31,51,57): both sides go through its two GEMMs (and their
        # backward) as a single 2*bz batch, user rows first
        # cat((local, global), 1) per tower (dual_att.py:50,56), user rows over item rows: one launch (RF.block_cat)
        if u_glo is None and i_glo is None:
            feats = self._fc(RF.stack_rows(u_loc, i_loc))                   # the merged conv's rows are the towers' cat already
        else:
            if u_glo is None:
                u_loc, u_glo = u_loc[:, :self.u_local_atten.out_size], u_loc[:, self.u_local_atten.out_size:]
            if i_glo is None:
                i_loc, i_glo = i_loc[:, :self.i_local_atten.out_size], i_loc[:, self.i_local_atten.out_size:]
            feats = self._fc(RF.block_cat(u_loc, u_glo, i_loc, i_glo))      # [2*bz, hidden_2], user rows first
        return RF.pair_dot(feats).view(-1)                                  # sum(u_feat * i_feat, 1)  (dual_att.py:58)

    def pair_latents(self, u_docs, i_docs):
        """forward's arguments -> (ul, il) [bz, hidden_size_2] each: the towers' latent rows -- the shared fc over both sides --
        under autograd and in the module's own train / eval mode (the fc keeps its dropout).  Same encoder pass as forward; the
        tail stops in front of the inner product, so that a loss over all bz x bz pairs of the batch
        (functional.pair_softmax_loss) can follow.  forward is untouched."""
        bz = u_docs.shape[0]
        pad = self.word_embeddings.padding_idx
        if self.validate_ids:
            u_docs, i_docs = RF.sanitize_ids([(u_docs, self.vocab_size, pad), (i_docs, self.vocab_size, pad)])
        u_par, i_par = self._tower_params(self.u_local_atten, self.u_global_atten), self._tower_params(self.i_local_atten, self.i_global_atten)
        feats = None
        if u_docs.shape == i_docs.shape and self.u_local_atten.window_size == self.i_local_atten.window_size:
            docs2 = RF.stack_rows(u_docs, i_docs)
            if RF.datt_pair_applies(self.word_embeddings.weight, docs2, u_par[0], u_par[4]):
                feats = self._fc(RF.datt_towers(self.word_embeddings.weight, docs2, u_par, i_par, padding_idx=pad,
                                                pad_runs=self.u_local_atten.window_size <= 17))
        if feats is None:
            tabs = RF.table_fanout(self.word_embeddings.weight, 8)
            u_loc, u_glo = self._encode(u_docs, self.u_local_atten, self.u_global_atten, tabs[0:4])
            i_loc, i_glo = self._encode(i_docs, self.i_local_atten, self.i_global_atten, tabs[4:8])
            if u_glo is None and i_glo is None:
                feats = self._fc(RF.stack_rows(u_loc, i_loc))
            else:
                if u_glo is None:
                    u_loc, u_glo = u_loc[:, :self.u_local_atten.out_size], u_loc[:, self.u_local_atten.out_size:]
                if i_glo is None:
                    i_loc, i_glo = i_loc[:, :self.i_local_atten.out_size], i_loc[:, self.i_local_atten.out_size:]
                feats = self._fc(RF.block_cat(u_loc, u_glo, i_loc, i_glo))
        return feats[:bz], feats[bz:]

    # ---- one tower at a time (recommend.Recommender): a tower reads its own documents only, the shared fc included
    def _encode_side(self, docs, local, glob):
        with RF.eval_mode(self):
            pad = self.word_embeddings.padding_idx
            if self.validate_ids:
                (docs,) = RF.sanitize_ids([(docs, self.vocab_size, pad)])
            loc, glo = self._encode(docs.contiguous(), local, glob, RF.table_fanout(self.word_embeddings.weight, 4))
            return self._fc(loc if glo is None else torch.cat((loc, glo), 1))       # cat((local, global), 1): dual_att.py:50,56

    def encode_users(self, u_docs):
        """u_docs [n, doc_len] int64 -> the users' latent rows [n, hidden_size_2] = fc(cat(local, global)) in eval semantics
        (dual_att.py:45-51), no autograd.  Any n: the item side is not needed."""
        return self._encode_side(u_docs, self.u_local_atten, self.u_global_atten)

    def encode_items(self, i_docs):
        """The item tower's counterpart of encode_users (dual_att.py:52-57)."""
        return self._encode_side(i_docs, self.i_local_atten, self.i_global_atten)

    # ---- why a pair scored as it did, through both gates (recommend.Recommender.attention)
    def _attend_side(self, docs, d_latent, local, glob):
        with RF.eval_mode(self):
            pad = self.word_embeddings.padding_idx
            if self.validate_ids:
                (docs,) = RF.sanitize_ids([(docs, self.vocab_size, pad)])
            docs, table = docs.contiguous(), self.word_embeddings.weight
            rows = RF.datt_token_rows(docs, table.shape[0])
            convs = [local.conv[0], glob.conv1[0], glob.conv2[0], glob.conv3[0]]
            weights, biases = [c.weight for c in convs], [c.bias for c in convs]
            runs = local.window_size <= 17
            gate_l = RF.datt_gate(table, local.attn[0].weight, local.attn[0].bias, docs, is_global=False, padding_idx=pad, rows=rows)
            gate_g = RF.datt_gate(table, glob.attn[0].weight, glob.attn[0].bias, docs, is_global=True, padding_idx=pad, rows=rows)
            if self._merged_applies(local, table, docs, weights, pad):
                feat, argmax = RF.textcnn(table, docs, None, weights, biases, gate=(gate_l, gate_g), gate_split=1,
                                          pad_mode=RF.PAD_VALID, act=RF.ACT_TANH, padding_idx=pad, pad_runs=runs, return_argmax=True)
            else:                                      # the two single-gate convs of the layers' encode, local channels first
                f_l, a_l = RF.textcnn(table, docs, None, weights[:1], biases[:1], gate=gate_l, pad_mode=RF.PAD_SAME, act=RF.ACT_TANH,
                                      padding_idx=pad, pad_runs=runs, return_argmax=True)
                f_g, a_g = RF.textcnn(table, docs, None, weights[1:], biases[1:], gate=gate_g, pad_mode=RF.PAD_VALID,
                                      act=RF.ACT_TANH, padding_idx=pad, pad_runs=True, return_argmax=True)
                feat, argmax = torch.cat((f_l, f_g), 1), torch.cat((a_l, a_g), 1)
            # the shared fc backwards: hid = relu(fc.0(feat)); d_feat = ((d_latent @ W2) * [hid > 0]) @ W1
            hid = RF.linear(feat, self.fc[0].weight, self.fc[0].bias, relu=True)
            d_hid = RF.linear(d_latent, self.fc[3].weight.t().contiguous()) * (hid > 0)
            d_feat = RF.linear(d_hid, self.fc[0].weight.t().contiguous())
            # a 1-wide 'same' conv is a 'valid' one: the four banks are one 'valid' conv for the saliency either way
            s = RF.datt_saliency(table, docs, (gate_l, gate_g), weights, feat, argmax, d_feat,
                                 (local.attn[0].weight, glob.attn[0].weight), gate_split=1, pad_mode=RF.PAD_VALID, act=RF.ACT_TANH)
            text = d_feat * feat
            k = local.out_size
            return gate_l, gate_g[:, 0].contiguous(), s.fixed + s.through, s.fixed, text[:, :k].sum(1), text[:, k:].sum(1)

    def attend_users(self, u_docs, d_latent):
        """u_docs [n, doc_len] int64 and d_latent [n, hidden_size_2] = d score / d (the users' latent rows) -> (local_gate [n, L],
        global_gate [n], tokens [n, L], tokens_fixed [n, L], local_text [n], global_text [n]) in eval semantics, no autograd.
        The gates are the forward's.  tokens[n, t] = <d score / d x[t], x[t]> for the embedded row x[t], followed through the
        shared fc, the four conv banks AND both gates, with only the max-pool routing held fixed (functional.datt_saliency);
        tokens_fixed is the part that reaches x[t] with the gates held constant, so tokens - tokens_fixed is what runs through the
        gates.  local_text / global_text = <d score / d feat, feat> over the local / global channels: what each half of the
        tower's features adds to the score through the fc."""
        return self._attend_side(u_docs, d_latent, self.u_local_atten, self.u_global_atten)

    def attend_items(self, i_docs, d_latent):
        """The item tower's counterpart of attend_users."""
        return self._attend_side(i_docs, d_latent, self.i_local_atten, self.i_global_atten)

    def explain_users(self, *args, **kwargs):
        """Not covered: the token-level explanation reads the un-gated TextCNN's max-pool routing."""
        raise ValueError("explain_users / explain_items cover DeepCoNN++ and NARRE with arch='CNN'; D-ATT is not covered")

    explain_items = explain_users

    def score_mode_and_params(self):
        """(mode, h, g, ub, ib) of functional.pair_score*: the plain inner product of the two latent rows (dual_att.py:58)."""
        return "dot", None, None, None, None
