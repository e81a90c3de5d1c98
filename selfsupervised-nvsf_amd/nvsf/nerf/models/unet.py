"""The ray-drop refinement U-Net (the reference's nvsf/nerf/models/unet.py) as a torch module: the specification of
csrc/unet.hip on CPU, the trainable form for RaydropRefiner.fit_tensors, and the yardstick the kernels are tested against.

Written from the reference's state-dict schema (tests/golden/network_state_dict_keys.json, `unet.*`) so that its checkpoints
load: module and attribute names below ARE the schema.

    inc    1 x 1 convolution with bias, in_channels -> c
    down   MaxPool2d(2) (floor), then a block                    c -> 2c -> 4c -> 8c -> 8c
    attn   at the bottom: 8 heads over 8c channels, residual
    up     bilinear x 2 (align_corners), zero pad to the skip's size (left / top get diff // 2), concat [skip, upsampled],
           then a block whose middle width is its input width     16c -> 4c, 8c -> 2c, 4c -> c, 2c -> c
    outc   BatchNorm, ReLU, 1 x 1 convolution with bias; then a sigmoid
    block  (BatchNorm -> ReLU -> Dropout2d(0.1) -> 3 x 3 convolution, padding 1, no bias) twice: normalisation FIRST
"""
import torch
import torch.nn.functional as F
from torch import nn


def _block(cin, cout, cmid=None, dropout=0.1):
    cmid = cmid or cout
    return nn.Sequential(nn.BatchNorm2d(cin), nn.ReLU(inplace=True), nn.Dropout2d(dropout), nn.Conv2d(cin, cmid, 3, padding=1, bias=False),
                         nn.BatchNorm2d(cmid), nn.ReLU(inplace=True), nn.Dropout2d(dropout), nn.Conv2d(cmid, cout, 3, padding=1, bias=False))


class _Block(nn.Module):
    def __init__(self, cin, cout, cmid=None):
        super().__init__()
        self.double_conv = _block(cin, cout, cmid)

    def forward(self, x):
        return self.double_conv(x)


class _In(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        return self.conv(x)


class _Out(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Sequential(nn.BatchNorm2d(cin), nn.ReLU(inplace=True), nn.Conv2d(cin, cout, 1))

    def forward(self, x):
        return self.conv(x)


class _Down(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = _Block(cin, cout)

    def forward(self, x):
        return self.conv(F.max_pool2d(x, 2))


class _Up(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = _Block(cin, cout, cin)

    def forward(self, low, skip):
        low = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
        dy, dx = skip.shape[2] - low.shape[2], skip.shape[3] - low.shape[3]
        low = F.pad(low, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
        return self.conv(torch.cat([skip, low], dim=1))


class _Attention(nn.Module):
    """Multi-head attention over the pixels.  The [B, heads, HW, C / heads] result is REINTERPRETED (view, no permute) as
    [B, H, W, C] before it is permuted to [B, C, H, W]: heads, pixels and channels mix.  That is what the reference computes, so it
    is what its trained checkpoints expect.  In training mode -1e12 is added to a Bernoulli(dropout) subset of the logits."""

    def __init__(self, channels, num_head=8, dropout=0.1):
        super().__init__()
        self.proj_qkv = nn.Conv2d(channels, 3 * channels, 1, bias=False)
        self.proj = nn.Conv2d(channels, channels, 1, bias=False)
        self.norm = nn.BatchNorm2d(channels)
        self.num_head, self.dropout = num_head, dropout

    def attend(self, x):
        B, C, H, W = x.shape
        q, k, v = self.proj_qkv(self.norm(x)).chunk(3, dim=1)
        q = q.reshape(B, self.num_head, -1, H * W).transpose(2, 3)
        k = k.reshape(B, self.num_head, -1, H * W)
        v = v.reshape(B, self.num_head, -1, H * W).transpose(2, 3)
        w = torch.matmul(q, k) * (C // self.num_head) ** -0.5
        if self.training:
            w = w + torch.bernoulli(torch.full_like(w, self.dropout)) * -1e12
        h = torch.matmul(F.softmax(w, dim=-1), v)             # [B, heads, HW, C / heads], contiguous
        return h.reshape(B, H, W, C).permute(0, 3, 1, 2)

    def forward(self, x):
        return x + self.proj(self.attend(x))


class UNet(nn.Module):
    def __init__(self, in_channels=3, channels=32, out_channels=1):
        super().__init__()
        c = channels
        self.in_channels, self.channels, self.out_channels = in_channels, channels, out_channels
        self.inc = _In(in_channels, c)
        self.down1, self.down2, self.down3, self.down4 = _Down(c, 2 * c), _Down(2 * c, 4 * c), _Down(4 * c, 8 * c), _Down(8 * c, 8 * c)
        self.attn = _Attention(8 * c)
        self.up1, self.up2, self.up3, self.up4 = _Up(16 * c, 4 * c), _Up(8 * c, 2 * c), _Up(4 * c, c), _Up(2 * c, c)
        self.outc = _Out(c, out_channels)

    def forward(self, x, return_attention=False):
        x0 = self.inc(x)
        x1 = self.down1(x0)
        x2 = self.down2(x1)
        x3 = self.down3(x2)
        x4 = self.attn(self.down4(x3))
        y = self.up4(self.up3(self.up2(self.up1(x4, x3), x2), x1), x0)
        p = torch.sigmoid(self.outc(y))
        return (p, x4) if return_attention else p
