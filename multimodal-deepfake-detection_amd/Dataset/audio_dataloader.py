"""MFCC clip dataset (reference: audio_dataloader.py:6-47).

``.npy`` MFCC arrays ``[T, 13]`` (T = 120 in wavfake_audio_dataset.py), label from the
file-name prefix, expanded to ``[T, 3, 13]`` by repeating the coefficient row over 3
channels (audio_dataloader.py:25-26); ``collate_fn`` zero-pads T to the batch maximum
giving ``[B, T, 3, 13]``.  File order is sorted.

``WaveDataset`` / ``collate_wave`` / ``get_wave_dataloader`` are the same for raw audio: ``.npy``
waveforms, int16 or fp32 ``[n]`` (what wavfake_audio_dataset.py:43 feeds librosa), zero-padded to the
batch maximum with the sample counts beside them, for ``xcp.WaveFrontEnd`` to turn into MFCC frames on
the GPU.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset


class AudioDataset(Dataset):
    def __init__(self, folder_path):
        self.folder_path = folder_path
        self.npy_files = sorted(os.path.join(folder_path, f) for f in os.listdir(folder_path) if f.endswith(".npy"))

    def __len__(self):
        return len(self.npy_files)

    def __getitem__(self, idx):
        npy_file = self.npy_files[idx]
        mfcc = np.load(npy_file, allow_pickle=False)
        label = 0 if os.path.basename(npy_file).split("_")[0].lower() == "real" else 1
        mfcc = torch.tensor(mfcc, dtype=torch.float32).unsqueeze(1).repeat(1, 3, 1)
        return mfcc, torch.tensor([label], dtype=torch.float32)


def collate_fn(batch):
    mfccs, labels = zip(*batch)
    max_seq_len = max(m.size(0) for m in mfccs)
    padded = torch.zeros((len(mfccs), max_seq_len, 3, mfccs[0].shape[-1]), dtype=torch.float32)
    for i, m in enumerate(mfccs):
        padded[i, :m.size(0)] = m
    return padded, torch.stack(labels)


def get_audio_dataloader(folder_path, batch_size=1, shuffle=False, num_workers=0):
    return DataLoader(AudioDataset(folder_path), batch_size=batch_size, shuffle=shuffle, collate_fn=collate_fn,
                      num_workers=num_workers)


class WaveDataset(Dataset):
    """``.npy`` waveforms, int16 or fp32 ``[n]``; labels and order as ``AudioDataset``."""

    def __init__(self, folder_path):
        self.folder_path = folder_path
        self.npy_files = sorted(os.path.join(folder_path, f) for f in os.listdir(folder_path) if f.endswith(".npy"))

    def __len__(self):
        return len(self.npy_files)

    def __getitem__(self, idx):
        npy_file = self.npy_files[idx]
        wav = np.load(npy_file, allow_pickle=False)
        if wav.ndim != 1 or wav.dtype not in (np.int16, np.float32):
            raise ValueError(f"{npy_file}: expected an int16 or fp32 [n] waveform, got {wav.dtype} {wav.shape}")
        label = 0 if os.path.basename(npy_file).split("_")[0].lower() == "real" else 1
        return torch.from_numpy(wav), torch.tensor([label], dtype=torch.float32)


def collate_wave(batch):
    """-> (wav [B, Nmax] zero-padded, int16 if every clip is int16, else fp32 with int16 clips as v / 32768;
    lengths int32 [B]; labels [B, 1])."""
    wavs, labels = zip(*batch)
    dtype = torch.int16 if all(w.dtype == torch.int16 for w in wavs) else torch.float32
    padded = torch.zeros((len(wavs), max(1, max(w.numel() for w in wavs))), dtype=dtype)
    for i, w in enumerate(wavs):
        padded[i, :w.numel()] = w if w.dtype == dtype else w.to(torch.float32) / 32768.0
    lengths = torch.tensor([w.numel() for w in wavs], dtype=torch.int32)
    return padded, lengths, torch.stack(labels)


def get_wave_dataloader(folder_path, batch_size=1, shuffle=False, num_workers=0):
    return DataLoader(WaveDataset(folder_path), batch_size=batch_size, shuffle=shuffle, collate_fn=collate_wave,
                      num_workers=num_workers)
