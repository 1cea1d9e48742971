"""Layer mirrors of models/ahn/ahn_layers.py (class names, constructor arguments, parameter names and initial-value bounds).

The HIP part is the encoder: Seq2SeqEncoder runs its bidirectional LSTM on csrc/lstm_seq.hip (functional.bilstm_encode), with
the input projection on the MFMA `linear`.  The hierarchical co-attention works on a few hundred rows per example and is, for
now, the TORCH COMPOSITION of the reference's arithmetic on whatever device its inputs live on; every such class says so."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import functional as RF
from ..deepconn.layers import WordEmbedding as _WordEmbedding
from ..simple_siamese.layers import VariationalDropout

MASK_FILL = -1e8          # the reference's fill of masked scores (utils.py:13, ahn_layers.py:522,534)


def masked_softmax(input_scores, input_masks):
    """utils.py:4-13 -- softmax over the last dimension of the scores with -1e8 at the masked places (torch composition)."""
    return F.softmax(torch.masked_fill(input_scores, ~input_masks, MASK_FILL), dim=-1)


def attention_weighted_sum(input_weights, inputs):
    """utils.py:15-28 -- sum over the sequence of weights [bz, seq_len(, 1)] * inputs [bz, seq_len, dim] (torch composition)."""
    if input_weights.dim() == 2:
        input_weights = input_weights.unsqueeze(-1)
    return torch.sum(input_weights * inputs, dim=1)


class WordEmbedding(_WordEmbedding):
    """ahn_layers.py:41-56 -- nn.Embedding(V, D, padding_idx) table, optional pretrained rows; the lookup is the HIP row gather
    (functional.embedding), whose backward builds the word table's gradient."""


class Seq2SeqEncoder(nn.Module):
    """ahn_layers.py:213-314 for the configuration AHN uses: one bidirectional nn.LSTM layer with biases, run over padded
    sequences as a packed sequence would be (lengths clamped to >= 1 by the reference, rows of length 0 zeroed).  `_encoder`
    is an nn.LSTM kept purely as the parameter container (state_dict keys `_encoder.weight_ih_l0`, ..., `_l0_reverse`); the
    arithmetic is HIP: functional.bilstm_encode (csrc/lstm_seq.hip)."""

    def __init__(self, rnn_type, input_size, hidden_size, num_layers=1, bias=True, dropout=0.0, bidirectional=False):
        super().__init__()
        covered = "covered: rnn_type=nn.LSTM, num_layers=1, bias=True, bidirectional=True"
        if not (isinstance(rnn_type, type) and issubclass(rnn_type, nn.RNNBase)):
            raise ValueError(f"rnn_type must be a class inheriting from torch.nn.RNNBase ({covered})")
        if rnn_type is not nn.LSTM or num_layers != 1 or not bias or not bidirectional:
            raise ValueError(f"Seq2SeqEncoder({rnn_type.__name__}, num_layers={num_layers}, bias={bias}, bidirectional={bidirectional}) "
                             f"has no HIP path ({covered})")
        if hidden_size > 256:
            raise ValueError(f"hidden_size {hidden_size} per direction exceeds the 256 the LSTM kernels cover")
        self.rnn_type, self.input_size, self.hidden_size = rnn_type, input_size, hidden_size
        self.num_layers, self.bias, self.bidirectional = num_layers, bias, bidirectional
        self.dropout = VariationalDropout(p=dropout) if dropout else None
        self._encoder = rnn_type(input_size, hidden_size, num_layers=num_layers, bias=bias, batch_first=True,
                                 bidirectional=bidirectional)

    def lstm_params(self):
        e = self._encoder
        return (e.weight_ih_l0, e.weight_hh_l0, e.bias_ih_l0, e.bias_hh_l0,
                e.weight_ih_l0_reverse, e.weight_hh_l0_reverse, e.bias_ih_l0_reverse, e.bias_hh_l0_reverse)

    def _dropped(self, sequences_batch, drop=None):
        """The reference's VariationalDropout in front of the LSTM: one [N, E] multiplier per sequence, shared over time.
        `drop`: a multiplier drawn by the caller (tests) instead of a fresh one."""
        if drop is None and self.dropout is not None:
            drop = self.dropout.multiplier(sequences_batch.shape[0], sequences_batch.shape[-1], sequences_batch.device)
        return sequences_batch if drop is None else drop.unsqueeze(1) * sequences_batch

    def forward(self, sequences_batch, sequences_lengths, drop=None):
        """sequences_batch [N, T, E], sequences_lengths int64 [N] -> [N, t_out, 2 * hidden_size] with t_out the batch's longest
        (clamped) length, as pad_packed_sequence trims it: one host synchronisation, exactly where the reference has one."""
        x = self._dropped(sequences_batch, drop)
        lengths = sequences_lengths.to(torch.int64)
        out = RF.bilstm_encode(x, self.lstm_params(), lengths, pool=False)
        t_out = int(lengths.clamp(1, min(x.shape[1], RF.LSTM_MAX_LEN)).max())
        return out[:, :t_out]

    def encode_max(self, sequences_batch, sequences_lengths, t_out=None, drop=None):
        """torch.max(self(sequences_batch, sequences_lengths), dim=1)[0] -> [N, 2 * hidden_size] in one HIP launch after the
        input projection, without a host synchronisation (ahn_model.py:62-67).  t_out: device int32, one value or one per
        sequence (default: this batch's own output length, computed on the device)."""
        x = self._dropped(sequences_batch, drop)
        pooled, _ = RF.bilstm_encode(x, self.lstm_params(), sequences_lengths.to(torch.int64), pool=True, t_out=t_out)
        return pooled


class Embedding(nn.Module):
    """ahn_layers.py:318-340 -- id embedding, uniform(+-1/sqrt(dim)) over every row, optional dropout (torch composition)."""

    def __init__(self, vocab_size, embedding_dim, dropout=0., padding_idx=0):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.embedding = nn.Embedding(vocab_size, embedding_dim, padding_idx=padding_idx)
        self.dropout = nn.Dropout(p=dropout) if dropout else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1. / math.sqrt(self.embedding_dim)
        nn.init.uniform_(self.embedding.weight, -bound, bound)

    def forward(self, inputs):
        out = self.embedding(inputs)
        return out if self.dropout is None else self.dropout(out)


class GatedAttention(nn.Module):
    """ahn_layers.py:482-542 -- gated attention pooling: scores = proj(tanh(W_t x) * sigmoid(W_g x)), softmax with -1e8 at the
    masked places, weighted sum.  With batch_contains_review the rows are (example, review) pairs and a SECOND softmax runs over
    all review_num * seq_len sentences of an example.  Torch composition; the HIP part of the model is the encoder."""

    def __init__(self, in_features, out_features, dropout=0.0, batch_contains_review=False, review_num=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.batch_contains_review, self.review_num = batch_contains_review, review_num
        self.dropout = nn.Dropout(p=dropout) if dropout else None
        self.trans_layer = nn.Sequential(nn.Linear(in_features, out_features, bias=False), nn.Tanh())
        self.gate_layer = nn.Sequential(nn.Linear(in_features, out_features, bias=False), nn.Sigmoid())
        self.proj_layer = nn.Linear(out_features, 1, bias=False)

    def forward(self, inputs, input_masks):
        """inputs [bz, seq_len, in_features], input_masks bool [bz, seq_len] -> (outputs [bz, in_features], att_weights
        [bz, seq_len]); with batch_contains_review: (outputs [bz / review_num, review_num, out_features], att_weights
        [bz / review_num, review_num, seq_len], review_unfolded_att_weights [bz / review_num, review_num * seq_len])."""
        att_scores = self.proj_layer(self.trans_layer(inputs) * self.gate_layer(inputs)).squeeze(-1)
        att_weights = masked_softmax(att_scores, input_masks)
        outputs = torch.sum(att_weights.unsqueeze(2) * inputs, dim=1)
        if self.dropout is not None:
            outputs = self.dropout(outputs)
        if not self.batch_contains_review:
            return outputs, att_weights
        if self.review_num is None:
            raise ValueError("GatedAttention(batch_contains_review=True) needs review_num (AHN: item_review_num)")
        seq_len = att_weights.size(-1)
        unfolded = masked_softmax(att_scores.view(-1, self.review_num * seq_len), input_masks.view(-1, self.review_num * seq_len))
        batch_size = inputs.size(0) // self.review_num
        return (outputs.view(batch_size, self.review_num, self.out_features), att_weights.view(batch_size, self.review_num, seq_len),
                unfolded)


class BiLinearInteraction(nn.Module):
    """ahn_layers.py:736-767 -- A = X W Y^T: X [bz, a, dim], Y [bz, b, dim], W [dim, dim] uniform(+-1/sqrt(dim)) -> [bz, a, b]
    (torch composition)."""

    def __init__(self, feat_dim, bias=False):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(feat_dim, feat_dim))
        if bias:
            self.bias = nn.Parameter(torch.empty(1))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1. / math.sqrt(self.weight.size(0))
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, input1, input2):
        y = torch.bmm(torch.matmul(input1, self.weight), input2.transpose(1, 2))
        return y if self.bias is None else y + self.bias


class UnbalancedCoAttentionAggregatorReview(nn.Module):
    """ahn_layers.py:562-588 -- reviews -> user / item: the item side by GatedAttention, the user side by the softmax of each
    user review's MAX bilinear similarity to the item's reviews.  Torch composition; the HIP part of the model is the encoder."""

    def __init__(self, in_features, out_features, interaction_type="BILINEAR"):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.item_aggregator = GatedAttention(in_features, out_features)
        self.bilinear = BiLinearInteraction(out_features, bias=False)

    def forward(self, user_review_inputs, item_review_inputs, user_review_masks, item_review_masks):
        item_outputs, item_review_weights = self.item_aggregator(item_review_inputs, item_review_masks)
        scores = self.bilinear(user_review_inputs, item_review_inputs)
        user_review_scores, _ = torch.max(scores, dim=2)
        user_review_weights = masked_softmax(user_review_scores, user_review_masks)
        user_outputs = attention_weighted_sum(user_review_weights, user_review_inputs)
        return user_outputs, item_outputs, user_review_weights, item_review_weights


class UnbalancedCoAttentionAggregator(nn.Module):
    """ahn_layers.py:590-660 -- sentences -> reviews.  The item's sentences are pooled per review by GatedAttention (softmax per
    review), and weighted by a second softmax over ALL of the item's sentences before the user side looks at them: each user
    sentence scores the MAX of its bilinear similarity to those weighted item sentences, and a masked softmax over the sentences
    of a user review pools them.  The reference loops over the user's reviews; here all of them go through one batched product
    (the same arithmetic per review).  Torch composition; the HIP part of the model is the encoder."""

    def __init__(self, in_features, out_features, item_review_num, interaction_type="BILINEAR"):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.interaction_type = interaction_type
        self.item_aggregator = GatedAttention(in_features, out_features, batch_contains_review=True, review_num=item_review_num)
        self.bilinear = BiLinearInteraction(in_features, bias=False)

    def forward(self, user_sent_inputs, item_sent_inputs, user_sent_masks, item_sent_masks, debug=False):
        """user_sent_inputs [bz, ur_num, us_num, F], item_sent_inputs [bz, ir_num, is_num, F], masks bool without the F ->
        (user_review_outputs [bz, ur_num, F], item_review_outputs [bz, ir_num, F], user_sent_weights [bz, ur_num, us_num],
        item_sent_weights [bz, ir_num, is_num], item_all_sent_weights [bz, ir_num * is_num])."""
        bz, ir_num, is_num, feat = item_sent_inputs.shape
        item_rows = item_sent_inputs.reshape(bz * ir_num, is_num, feat)
        item_review_outputs, item_sent_weights, item_all_sent_weights = self.item_aggregator(
            item_rows, item_sent_masks.reshape(bz * ir_num, is_num))
        item_all = item_rows.view(bz, ir_num * is_num, feat) * item_all_sent_weights.unsqueeze(-1)
        _, ur_num, us_num, _ = user_sent_inputs.shape
        scores = self.bilinear(user_sent_inputs.reshape(bz, ur_num * us_num, feat), item_all)        # [bz, ur*us, ir*is]
        user_sent_scores, _ = torch.max(scores, dim=2)
        user_sent_weights = masked_softmax(user_sent_scores.view(bz, ur_num, us_num), user_sent_masks)
        user_review_outputs = torch.sum(user_sent_weights.unsqueeze(-1) * user_sent_inputs, dim=2)
        return user_review_outputs, item_review_outputs, user_sent_weights, item_sent_weights, item_all_sent_weights


def glorot(shape):
    """ahn_layers.py:925-929 -- Glorot & Bengio uniform init."""
    init_range = math.sqrt(6.0 / (shape[0] + shape[1]))
    return (2 * init_range) * torch.rand(shape[0], shape[1]) - init_range


class TorchFM(nn.Module):
    """ahn_layers.py:932-947 -- factorization machine 0.5 * ((x V)^2 - x^2 V^2).sum + lin(x) -> [bz, 1] (torch composition)."""

    def __init__(self, n=None, k=None):
        super().__init__()
        self.V = nn.Parameter(glorot([n, k]), requires_grad=True)
        self.lin = nn.Linear(n, 1)

    def forward(self, x):
        out_1 = torch.matmul(x, self.V).pow(2).sum(1, keepdim=True)
        out_2 = torch.matmul(x.pow(2), self.V.pow(2)).sum(1, keepdim=True)
        return 0.5 * (out_1 - out_2) + self.lin(x)
