"""TEST INFRASTRUCTURE: the reference's PIT SI-SNR loss (src/loss/ss_losses.py:21-26 batch-level PIT, :100-114 SiSNRLoss)
restated in stock PyTorch, differentiable, for tests/test_convtasnet_train_host.py."""
from __future__ import annotations

import torch


def _sisnr_loss(pred, gt):
    pred = pred - pred.mean(dim=-1, keepdim=True)
    gt = gt - gt.mean(dim=-1, keepdim=True)
    scaled = (gt * pred).sum(dim=-1, keepdim=True) / (torch.linalg.norm(gt, ord=2, dim=-1, keepdim=True) ** 2) * gt
    noise = pred - scaled
    sig = torch.linalg.norm(scaled, ord=2, dim=-1, keepdim=True) ** 2
    nz = torch.linalg.norm(noise, ord=2, dim=-1, keepdim=True) ** 2
    return (-20 * torch.log10(sig / nz)).mean()


def pit_sisnr_loss(s1_pred, s2_pred, s1, s2):
    l1 = (_sisnr_loss(s1_pred, s1) + _sisnr_loss(s2_pred, s2)) / 2
    l2 = (_sisnr_loss(s1_pred, s2) + _sisnr_loss(s2_pred, s1)) / 2
    return l2 if l2 < l1 else l1
