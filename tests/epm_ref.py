"""fp64 restatement of the EPM baseline's adversarial pieces, written from their formulas (not from the reference's text):

  centre-aware map    atten = sigmoid(w * max_c sigmoid(cls[., c]) * sigmoid(ctr))
  GA discriminator    x -> n x [conv3x3 + bias, GroupNorm(32, eps 1e-5), ReLU] -> conv3x3 256 -> 1 -> mean_m bce(logit_m, t)
  CA discriminator    'ca_feature': the GA discriminator on atten * x;  'ca_loss': mean_m atten_m * bce(logit_m, t)

with bce(z, t) = max(z, 0) - z t + log(1 + exp(-|z|)).  The gradient-reversal layer in front of the tower is the identity
forward and multiplies the gradient by -lambda, so d loss / d feature here carries that factor.  Everything is torch float64 on
the CPU; NCHW in and out.
"""
import torch
import torch.nn.functional as F


def center_aware_map(cls, ctr, weight):
    """cls [..., C] logits (classes last), ctr [...] -> atten [...] in float64"""
    p = torch.sigmoid(cls.double()).amax(-1)
    return torch.sigmoid(float(weight) * p * torch.sigmoid(ctr.double()))


def center_aware_map_fp32(cls, ctr, weight):
    """the same formula evaluated operation by operation in float32 (what an fp32 framework computes): the yardstick for the
    kernel's own rounding error"""
    p = torch.sigmoid(cls.float()).amax(-1)
    return torch.sigmoid(torch.tensor(float(weight), dtype=torch.float32) * p * torch.sigmoid(ctr.float()))


def bce(z, t):
    return z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))


def tower_logits(x, sd, num_convs):
    """x [N, 256, h, w] float64, sd: state_dict (dis_tower.{3i, 3i+1}.*, cls_logits.*) -> logits [N, 1, h, w]"""
    for i in range(num_convs):
        x = F.conv2d(x, sd["dis_tower.%d.weight" % (3 * i)].double(), sd["dis_tower.%d.bias" % (3 * i)].double(), padding=1)
        x = F.relu(F.group_norm(x, 32, sd["dis_tower.%d.weight" % (3 * i + 1)].double(),
                                sd["dis_tower.%d.bias" % (3 * i + 1)].double(), eps=1e-5))
    return F.conv2d(x, sd["cls_logits.weight"].double(), sd["cls_logits.bias"].double(), padding=1)


def discriminator(feature, sd, num_convs, target, lam, kind="ga", box_cls=None, centerness=None, weight=0.0):
    """-> (loss, d loss / d feature through the GRL) in float64.  kind: 'ga' | 'ca_feature' | 'ca_loss'; box_cls [N, C, h, w]
    and centerness [N, 1, h, w] for the CA kinds."""
    x = feature.double().clone().requires_grad_(True)
    atten = None
    if kind != "ga":
        atten = center_aware_map(box_cls.permute(0, 2, 3, 1), centerness[:, 0], weight)[:, None]  # [N, 1, h, w]
    z = tower_logits(atten * x if kind == "ca_feature" else x, sd, num_convs)
    l = bce(z, float(target))
    loss = (atten * l).mean() if kind == "ca_loss" else l.mean()
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), -float(lam) * g
