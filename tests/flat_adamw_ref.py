"""float64 restatement of what optim.FlatAdamW computes (include/fastmax_hip_optim.h), shared by the FlatAdamW tests:
torch.optim.AdamW with amsgrad=False, maximize=False over one flat range, with the division by the world size (grad_scale) and
torch's clip_grad_norm_ coefficient in front."""
import numpy as np

# max |error| of a float32 parameter or master after 6 steps at lr = 1e-2 and |p| <= 0.5 against this restatement:
# the float32 rounding of p gives 6 * 0.5 * 2^-24 = 1.8e-7, the update term at most about 100 ulp * lr = 6e-8 per step
PARITY_TOL = 1e-6


class AdamWRef:
    def __init__(self, p0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.p = np.asarray(p0, dtype=np.float64).copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.norm = self.coef = None

    def step(self, g, grad_scale=1.0, max_norm=None, lr=None):
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        g = np.asarray(g, dtype=np.float64) * grad_scale
        if max_norm is not None:
            self.norm = float(np.sqrt((g * g).sum()))
            self.coef = min(1.0, max_norm / (self.norm + 1e-6))
            g = g * self.coef
        self.t += 1
        self.p *= 1.0 - lr * self.wd
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        self.p -= (lr / bc1) * self.m / (np.sqrt(self.v) / np.sqrt(bc2) + self.eps)
        return self.p
