"""Visual clip model (XceptionLSTMV.py:9-70): frozen Xception per frame -> LSTM -> FC head.

Same constructor, submodules (``feature_extractor``, ``lstm``, ``fc_layers``,
``fc_out``, ``sigmoid``), init order and state_dict as the reference.  The
backbone runs on the xcp engine (one pass over the B*T frame batch, temporal
batching as XceptionLSTMV.py:55), ``lstm`` is the fused-kernel ``nn.LSTM``
drop-in; the small FC head stays on PyTorch-ROCm (hipBLASLt).

``pretrained`` defaults to True as in the reference (XceptionLSTMV.py:12); offline
that needs a local weight file (see ``Models.Xception.xception``).
"""
import torch
import torch.nn as nn

from xcp.lstm import LSTM

from .Xception import xception


class XceptionLSTMV(nn.Module):
    def __init__(self, hidden_dim, pretrained=True, bidirectional=False):
        """``bidirectional=True``: ``lstm`` reads each clip in both directions of time and the head is fed
        ``cat(h_n[0], h_n[1])`` (the forward state after the clip's last frame, the reverse state after its
        first), so ``fc_layers[0]`` is ``Linear(2 * hidden_dim, 1024)``.  The default is the reference's model,
        unchanged."""
        super(XceptionLSTMV, self).__init__()
        self.feature_extractor = xception(pretrained=pretrained)
        self.feature_extractor.fc = nn.Identity()
        for param in self.feature_extractor.parameters():
            param.requires_grad = False
        self.bidirectional = bool(bidirectional)
        if self.bidirectional:
            self.lstm = LSTM(input_size=2048, hidden_size=hidden_dim, num_layers=1, batch_first=True,
                             bidirectional=True)
        else:
            self.lstm = LSTM(input_size=2048, hidden_size=hidden_dim, num_layers=1, batch_first=True)
        self.fc_layers = nn.Sequential(
            nn.Linear(2 * hidden_dim if self.bidirectional else hidden_dim, 1024), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(1024, 1024), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(1024, 1024), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(1024, 1024), nn.ReLU(), nn.Dropout(0.3),
        )
        self.fc_out = nn.Linear(1024, 1)
        self.sigmoid = nn.Sigmoid()

    def extract_features(self, video_batch, device=None):
        """[B,T,3,H,W] -> [B,T,2048] (XceptionLSTMV.py:46-63).  ``device`` may also be the
        ``seq_lengths`` tensor the active train_visual.py:568 passes.  The backbone ignores it
        and runs over the padded frames too, as the reference does (dropping frames would change
        every BatchNorm's batch statistics); ``forward(features, seq_lengths)`` honours it."""
        if device is not None and not torch.is_tensor(device):
            self.feature_extractor.to(device)
        batch_size, seq_len, c, h, w = video_batch.shape
        frames = video_batch.reshape(batch_size * seq_len, c, h, w)
        frame_features = self.feature_extractor(frames)
        return frame_features.view(batch_size, seq_len, -1)

    def forward(self, features, seq_lengths=None):
        """``features`` [B,T,2048] -> clip probability [B,1].  With ``seq_lengths`` ([B], the loaders'
        per-clip frame counts of the zero-padded batch; train_visual.py:111) the head is fed the LSTM
        state at each clip's own last frame instead of the state after the padding."""
        if self.bidirectional:   # both summaries: forward after the last real frame, reverse after the first
            _, (h_n, _) = self.lstm(features, lengths=seq_lengths)
            lstm_out = torch.cat((h_n[0], h_n[1]), dim=1)
        elif seq_lengths is not None:
            _, (h_n, _) = self.lstm(features, lengths=seq_lengths)
            lstm_out = h_n[0]
        else:
            lstm_out, _ = self.lstm(features)
            lstm_out = lstm_out[:, -1, :]
        dense_out = self.fc_layers(lstm_out)
        return self.sigmoid(self.fc_out(dense_out))

    def forward_state(self, features, seq_lengths=None, state=None):
        """``forward`` for a clip that arrives in chunks of frames: ``state`` is the ``(h, c)`` pair (each
        [1,B,H]) the previous chunk returned, or None at the clip's start; returns ``(prob, (h_n, c_n))`` with
        the probability of the clip so far.  A clip with no frame in this chunk (device ``seq_lengths`` entry
        0) keeps its state, so its probability stays that of its last real frame.  ``forward`` keeps its
        two-argument signature (tests pin it), so the state has a method of its own."""
        if self.bidirectional:
            raise ValueError("forward_state: a bidirectional model cannot be fed in chunks of frames (its reverse "
                             "direction starts from the clip's last frame); use forward on the whole clip")
        _, (h_n, c_n) = self.lstm(features, state, lengths=seq_lengths)
        dense_out = self.fc_layers(h_n[0])
        return self.sigmoid(self.fc_out(dense_out)), (h_n, c_n)
