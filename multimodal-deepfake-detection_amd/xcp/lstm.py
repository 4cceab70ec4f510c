"""``nn.LSTM`` drop-in whose forward/backward run on the xcp kernels.

Reference: the single-layer, batch_first ``nn.LSTM(2048, H)`` of
XceptionLSTMV.py:18-23 / XceptionLSTMA.py:14-19, used as ``self.lstm(features)``
(XceptionLSTMV.py:67) and as ``model.lstm(features)[0][:, -1, :]``
(train_visual.py:569).  Subclassing ``nn.LSTM`` keeps the parameter names
(``weight_ih_l0`` ...), the init (uniform(-1/sqrt(H), 1/sqrt(H)), same RNG
consumption) and the state_dict, so reference checkpoints load unchanged.

The computation is the ``torch.ops.xcp.lstm`` custom op (xcp/torch_ops.py): the input
projection for all T steps is one fp32 MFMA GEMM, the recurrence one fused kernel per
direction of time (lstm.hip).  The head runs in fp32 in every precision mode (it is
~0.1 GFLOP per clip).

Zero-padded clips of unequal length (the loaders' ``seq_lengths``) go through
``torch.ops.xcp.lstm_varlen`` (the same kernels in lstm.hip), either as ``lstm(x, lengths=...)`` or as a
``PackedSequence`` input, with the semantics of ``pack_padded_sequence`` -> ``nn.LSTM`` ->
``pad_packed_sequence``.

An initial state ``hx = (h0, c0)`` goes through ``torch.ops.xcp.lstm_state`` (state-aware instantiations of
the same kernels), with or without lengths: a long clip can be fed in chunks of frames with the state
carried from one chunk to the next (xcp/streaming.py), and ``h0`` / ``c0`` are differentiable.

``bidirectional=True`` goes through ``torch.ops.xcp.lstm_bidir``: direction-aware instantiations of the same
kernels run the two directions of time in the same launches, the reverse one reading each clip backwards from
its own last frame, and write ``out [B, T, 2H]`` in place.
"""
import torch
import torch.nn as nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from . import torch_ops  # noqa: F401  (registers torch.ops.xcp.lstm, .lstm_varlen, .lstm_state)


class LSTM(nn.LSTM):
    """nn.LSTM with the xcp forward.  Supported configuration (the reference's):
    num_layers=1, batch_first=True, bias=True, proj_size=0, one or both directions of time.
    ``xcp_kernel`` (attribute): 0 = automatic recurrence kernel choice, 1 = the generic kernels.

    ``forward(input, hx=None, lengths=None)``: with ``lengths`` (int32 / int64 ``[B]``) clip ``b`` is
    ``input[b, :lengths[b]]`` and the rest of its rows is padding: ``out[b, t >= L]`` is zero, ``h_n`` /
    ``c_n`` are the state after the clip's last real frame and the padding receives and contributes no
    gradient.  Padded input rows must be finite (the loaders write zeros).  A CPU ``lengths`` tensor is
    validated (``1 <= L <= T``, as ``pack_padded_sequence`` demands); a device tensor is passed to the
    kernels unread -- they clamp it to ``[0, T]``, and a clip of length 0 gives zero outputs, states and
    gradients -- so the call stays capturable in a HIP graph.  A ``PackedSequence`` input is unpacked,
    run the same way and returned packed, with ``h_n`` / ``c_n`` in the caller's batch order.

    ``hx = (h0, c0)``, each floating ``[1, B, H]`` on the input's device as ``nn.LSTM`` takes them (for a
    ``PackedSequence`` in the caller's batch order), starts every clip from that state; both receive
    gradients.  The state is kept in fp32 whatever dtype it comes in.  With device lengths a clip of length
    0 hands its state on unchanged (``h_n = h0``, ``c_n = c0``, ``d/dh0 = d/dh_n``, ``d/dc0 = d/dc_n``), which
    is what carries a short clip's state through the later chunks of a batch.  A call with ``hx`` runs the
    register-resident, per-step or generic kernels, never the persistent ones; ``hx=None`` calls exactly the
    ops it always did.

    ``bidirectional=True`` (parameters ``weight_ih_l0_reverse`` ... as ``nn.LSTM`` names and initialises them, so
    its checkpoints load): returns ``(out [B, T, 2H], (h_n [2, B, H], c_n [2, B, H]))`` with the forward
    direction in ``out[..., :H]`` / ``h_n[0]`` and the reverse one in ``out[..., H:]`` / ``h_n[1]``, the state
    after the clip's first frame.  ``hx`` is ``[2, B, H]`` each; lengths, ``PackedSequence`` input and the
    length-0 rule work as above, per direction.  It never runs the persistent kernels either.  ``num_layers``
    stays 1: a deeper stack is a second ``LSTM(2 * H, H, bidirectional=True)`` module fed this one's ``out``."""

    xcp_kernel = 0

    def forward(self, input, hx=None, lengths=None):  # noqa: A002  (nn.LSTM signature)
        if self.num_layers != 1 or not self.batch_first or not self.bias or self.proj_size:
            raise NotImplementedError("xcp LSTM supports the reference configuration only "
                                      "(1 layer, batch_first, bias, no projection)")
        if isinstance(input, PackedSequence):
            if lengths is not None:
                raise ValueError("a PackedSequence carries its own lengths; do not pass lengths= with it")
            return self._forward_packed(input, hx)
        if input.dim() != 3:
            raise NotImplementedError("xcp LSTM expects batched [B, T, F] input")
        if lengths is not None:
            lengths = self._check_lengths(lengths, input.shape[0], input.shape[1])
        if hx is not None:
            h0, c0 = self._check_hx(hx, input)
        if not input.is_cuda:
            raise RuntimeError("xcp LSTM runs on the MI355X only (got a non-GPU tensor); there is no CPU fallback")
        if self.bidirectional:
            if lengths is not None:
                lengths = lengths.to(device=input.device, dtype=torch.int32).contiguous()
            out, hn, cn, _, _, _ = torch.ops.xcp.lstm_bidir(
                input, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                self.weight_ih_l0_reverse, self.weight_hh_l0_reverse, self.bias_ih_l0_reverse,
                self.bias_hh_l0_reverse, *((h0, c0) if hx is not None else (None, None)), lengths,
                int(self.xcp_kernel))
            return out.to(input.dtype), (hn, cn)
        if hx is not None:
            if lengths is not None:
                lengths = lengths.to(device=input.device, dtype=torch.int32).contiguous()
            out, hn, cn, _, _, _ = torch.ops.xcp.lstm_state(
                input, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0, h0, c0, lengths,
                int(self.xcp_kernel))
            return out.to(input.dtype), (hn, cn)
        if lengths is not None:
            out, hn, cn, _, _, _ = torch.ops.xcp.lstm_varlen(
                input, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0,
                lengths.to(device=input.device, dtype=torch.int32).contiguous(), int(self.xcp_kernel))
            return out.to(input.dtype), (hn, cn)
        out, hn, cn, _, _, _ = torch.ops.xcp.lstm(input, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0,
                                                  self.bias_hh_l0, int(self.xcp_kernel))
        return out.to(input.dtype), (hn, cn)

    @staticmethod
    def _check_lengths(lengths, B, T):
        if not torch.is_tensor(lengths) or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError("lengths must be an int32 or int64 tensor")
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"lengths must have shape [{B}] (one per clip), got {tuple(lengths.shape)}")
        if not lengths.is_cuda and B > 0:   # host values: pack_padded_sequence's rule; device values are clamped
            lo, hi = int(lengths.min()), int(lengths.max())
            if lo < 1 or hi > T:
                raise ValueError(f"lengths must lie in [1, {T}] (the padded length), got [{lo}, {hi}]")
        return lengths

    def _check_hx(self, hx, input):  # noqa: A002
        """(h0, c0), each floating [D, B, H] (D directions) on the input's device; refused in nn.LSTM's words
        where it has any"""
        if not isinstance(hx, (tuple, list)) or len(hx) != 2 or not all(torch.is_tensor(t) for t in hx):
            raise ValueError("hx must be a tuple of two tensors (h_0, c_0)")
        B, H = input.shape[0], self.hidden_size
        for i, t in enumerate(hx):
            if t.dim() != 3:
                raise RuntimeError("For batched 3-D input, hx and cx should also be 3-D but got "
                                   f"({hx[0].dim()}-D, {hx[1].dim()}-D) tensors")
            D = 2 if self.bidirectional else 1
            if tuple(t.shape) != (D, B, H):
                raise RuntimeError(f"Expected hidden[{i}] size {(D, B, H)}, got {list(t.shape)}")
            if not t.is_floating_point():
                raise ValueError(f"hx[{i}] must be a floating-point tensor, got {t.dtype}")
            if t.device != input.device:
                raise RuntimeError("Input and hidden tensors are not at the same device, found input tensor at "
                                   f"{input.device} and hidden tensor at {t.device}")
        return hx[0], hx[1]

    def _forward_packed(self, packed, hx=None):
        """Compatibility path: plain torch gathers around the length-aware op (hx, like h_n / c_n, is in the
        caller's batch order, which is the order the padded batch is run in)."""
        x, lens = pad_packed_sequence(packed, batch_first=True)   # caller's batch order, lens on the CPU
        out, (hn, cn) = self.forward(x, hx, lengths=lens)
        si = packed.sorted_indices
        if si is not None:
            out, lens = out.index_select(0, si), lens.index_select(0, si.to(lens.device))
        data = pack_padded_sequence(out, lens, batch_first=True, enforce_sorted=True).data
        return PackedSequence(data, packed.batch_sizes, packed.sorted_indices, packed.unsorted_indices), (hn, cn)
