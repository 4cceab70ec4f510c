"""Scoring a long clip in chunks of frames, with the LSTM state carried from chunk to chunk.

The backbone's activations grow with B*T frames, so a 300-frame video (the preprocessors write up to that
many) cannot go through a clip model in one piece.  The LSTM is the only part of the model that looks
across frames, and it can start from a given state (``xcp.lstm.LSTM.forward(input, hx)``): the frames are
fed ``chunk`` at a time, each chunk's ``(h_n, c_n)`` is the next chunk's ``hx``, and the head reads the
state after the last chunk.  Peak activation memory is one chunk's.
"""
import torch


def score_in_chunks(model, clips, seq_lengths=None, chunk=16):
    """Clip probabilities [B, 1] of a clip model with ``extract_features`` / ``lstm`` / ``fc_layers`` /
    ``fc_out`` / ``sigmoid`` (XceptionLSTMV), computed ``chunk`` frames at a time.

    clips: [B, T, 3, H, W] on the model's device; seq_lengths: the per-clip frame counts of a zero-padded
    batch ([B], int32 / int64, any device).  Chunk ``clips[:, off:off + chunk]`` gets the lengths
    ``(seq_lengths - off).clamp(0, chunk)``, formed on the device with no host read; a clip that has ended
    has length 0 there and the kernels hand its state on unchanged, so the head sees every clip's state at
    its own last frame.  The last chunk may be shorter.  The model runs in eval mode (running BatchNorm
    statistics, no dropout) under ``no_grad`` and gets its previous mode back, module by module; with
    ``chunk >= T`` this is the unchunked ``model(model.extract_features(clips), seq_lengths)``.  The
    backbone still runs over padded frames, as ``extract_features`` always does."""
    if clips.dim() != 5:
        raise ValueError("score_in_chunks: clips must be [B, T, 3, H, W]")
    if getattr(model.lstm, "bidirectional", False):
        raise ValueError("score_in_chunks: a bidirectional model cannot be scored in chunks (its reverse direction "
                         "needs the clip's future frames); score the whole clip with model(features, seq_lengths)")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("score_in_chunks: chunk must be at least 1 frame")
    if clips.shape[1] < 1:
        raise ValueError("score_in_chunks: clips have no frame")
    lens = None
    if seq_lengths is not None:
        if not torch.is_tensor(seq_lengths) or seq_lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError("seq_lengths must be an int32 or int64 tensor")
        if tuple(seq_lengths.shape) != (clips.shape[0],):
            raise ValueError(f"seq_lengths must have shape [{clips.shape[0]}] (one per clip), got "
                             f"{tuple(seq_lengths.shape)}")
        lens = seq_lengths.to(clips.device)
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            state = None
            for off in range(0, clips.shape[1], chunk):
                feats = model.extract_features(clips[:, off:off + chunk])
                _, state = model.lstm(feats, state, lengths=None if lens is None else (lens - off).clamp(0, chunk))
            return model.sigmoid(model.fc_out(model.fc_layers(state[0][0])))
    finally:
        for m, t in modes:
            m.training = t
