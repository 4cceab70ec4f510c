"""Audio clip model (XceptionLSTMA.py:5-59): MFCC frames resized to 64x64 -> Xception -> LSTM -> FC.

Same module surface as the reference.  ``extract_features`` reshapes
``[B,T,3,13]`` to ``[B*T,3,13,1]``, resizes bilinearly to 64x64
(align_corners=False, XceptionLSTMA.py:46) with the HIP kernel ``xcp_resize_bilinear``
and runs the xcp backbone.
"""
import torch
import torch.nn as nn
from xcp import ops
from xcp.lstm import LSTM

from .Xception import xception


class XceptionLSTMA(nn.Module):
    def __init__(self, hidden_dim, pretrained=True, bidirectional=False):
        """``bidirectional=True``: ``lstm`` reads each clip in both directions of time and the head is fed
        ``cat(h_n[0], h_n[1])`` (the forward state after the clip's last frame, the reverse state after its
        first), so ``fc_layers[0]`` is ``Linear(2 * hidden_dim, 1024)``.  The default is the reference's model,
        unchanged."""
        super(XceptionLSTMA, self).__init__()
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

    def extract_features(self, audio_batch, device=None):
        if device is not None and not torch.is_tensor(device):
            self.feature_extractor.to(device)
        batch_size, time_steps, c, n_mfcc = audio_batch.shape
        if torch.is_grad_enabled() and audio_batch.requires_grad:
            # (the backbone would return a gradient w.r.t. the resized frames, which would stop there, silently)
            raise NotImplementedError("XceptionLSTMA.extract_features: no gradient w.r.t. the MFCC input "
                                      "(xcp_resize_bilinear has no backward); detach it or run under torch.no_grad()")
        frames = audio_batch.reshape(batch_size * time_steps, c, n_mfcc, 1)
        frames = ops.resize_bilinear(frames, (64, 64))
        frame_features = self.feature_extractor(frames)
        return frame_features.view(batch_size, time_steps, frame_features.shape[-1])

    def input_frames(self, audio_batch):
        """The backbone's input for ``audio_batch`` [B,T,3,n_mfcc]: fp32 [B*T,3,64,64], the images
        ``extract_features`` feeds it (XceptionLSTMA.py:44-46).  ``xcp.grad_cam`` draws its maps over these."""
        batch_size, time_steps, c, n_mfcc = audio_batch.shape
        return ops.resize_bilinear(audio_batch.detach().reshape(batch_size * time_steps, c, n_mfcc, 1), (64, 64))

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
        the probability of the clip so far (see XceptionLSTMV.forward_state)."""
        if self.bidirectional:
            raise ValueError("forward_state: a bidirectional model cannot be fed in chunks of frames (its reverse "
                             "direction starts from the clip's last frame); use forward on the whole clip")
        _, (h_n, c_n) = self.lstm(features, state, lengths=seq_lengths)
        dense_out = self.fc_layers(h_n[0])
        return self.sigmoid(self.fc_out(dense_out)), (h_n, c_n)
