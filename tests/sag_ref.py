"""Self-attention guidance restated in float64, in plain torch (diffusers' StableDiffusionSAGPipeline in the sigma parametrisation of the SDXL Euler
step): the column mass of a self-attention, the degraded latents and the guided prediction.  Nothing of the kernels' tiling appears here."""
import math

import torch
import torch.nn.functional as F


def colmass(q, k, heads, batch, scale, dtype=torch.float64):
    """mass [batch, L]: the mean over heads of the column sums of softmax(q_h k_h^T * scale); q, k [batch * L, heads * 64]"""
    L = q.shape[0] // batch
    split = lambda t: t.to(dtype).reshape(batch, L, heads, 64).permute(0, 2, 1, 3)      # noqa: E731
    p = torch.softmax(split(q) @ split(k).transpose(-1, -2) * scale, dim=-1)
    return p.sum(dim=2).mean(dim=1)


def taps(blur_sigma):
    t = torch.exp(-0.5 * (torch.arange(-4, 5, dtype=torch.float64) / blur_sigma) ** 2)
    return t / t.sum()


def blur(x, blur_sigma):
    """depthwise 9 x 9 Gaussian under reflect padding of 4; x float64 [n, C, h, w]"""
    t, c = taps(blur_sigma), x.shape[1]
    x = F.pad(x, (4, 4, 4, 4), mode="reflect")
    x = F.conv2d(x, t.reshape(1, 1, 1, 9).expand(c, 1, 1, 9), groups=c)
    return F.conv2d(x, t.reshape(1, 1, 9, 1).expand(c, 1, 9, 1), groups=c)


def stretch(mask, h, w):
    """mask [n, h_m, w_m] to [n, 1, h, w] by nearest neighbour: element (y, x) reads (floor(y h_m / h), floor(x w_m / w))"""
    hm, wm = mask.shape[1:]
    ys, xs = torch.arange(h) * hm // h, torch.arange(w) * wm // w
    return mask[:, ys][:, :, xs].bool().unsqueeze(1)


def degrade(x, eps_u, sigma, mask, blur_sigma):
    """(x_deg, x0, n) in float64: x0 = x - sigma eps_u, x_deg = where(mask, blur(x0), x0) + sigma eps_u"""
    x, n = x.double(), sigma.double().reshape(-1, 1, 1, 1) * eps_u.double()
    x0 = x - n
    return torch.where(stretch(mask, *x.shape[2:]), blur(x0, blur_sigma), x0) + n, x0, n


def guided(eps_u, eps_c, eps_d, g, sag_scale):
    eps_u, eps_c, eps_d = eps_u.double(), eps_c.double(), eps_d.double()
    return eps_u + g * (eps_c - eps_u) + sag_scale * (eps_u - eps_d)


LN2 = math.log(2.0)
