"""DeviceNoise - the counter-based device noise stream (csrc/sw_noise.hip, sw_noise_uniform).

The reference draws z ~ U[0, 1) from torch's CPU generator (train.py:473, :584), and that host stream stays this package's
default.  A DeviceNoise makes z on the device instead: every value is a pure function of (seed, domain, step, draw, row,
column) - Philox4x32-10, include/socialways_hip.h has the specification -, so

  - a data-parallel rank or an evaluation chunk fills exactly its rows in one launch, whatever was drawn before;
  - evaluation repeats call to call and does not depend on how scenes are folded into launches;
  - {"seed", "step"} in a checkpoint continues the same training stream.

Domains: TRAIN (0) - step = index of the packed batch since the stream began, draw 0 = the step's z, draws 1 .. = the extra
samples of use_variety_loss="fixed", row = row in the global packed batch; EVAL (1) - step 0, draw = the k of the K samples,
row = the agent's row (the absolute held-out row in evaluate*()).
"""
import torch

from . import _lib as L

TRAIN, EVAL = 0, 1


class DeviceNoise:
    def __init__(self, seed, step=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF      # the key is 64 bits
        self.step = int(step)                            # training: packed batches drawn so far (every rank counts them all)

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, sd):
        self.seed = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.step = int(sd["step"])

    def __repr__(self):
        return "DeviceNoise(seed=%d, step=%d)" % (self.seed, self.step)

    def fill(self, rows, cols, *, domain, step=0, n_steps=1, draw0=0, n_draws=1, row0=0, ld=None, out=None, device="cuda"):
        """(n_steps, n_draws, rows, ld) fp32 on the device: [t, k, i, j] = the stream's value at (step + t, draw0 + k,
        row0 + i, j) for j < cols, 0 in the padding columns cols .. ld-1 (ld: default cols rounded up to 4).  One launch on
        the current stream, no host sync.  `out`: a contiguous fp32 device tensor of that many elements to fill instead
        of a new one (returned viewed in that shape).  There is no host implementation: a CPU device raises."""
        rows, cols, n_steps, n_draws = int(rows), int(cols), int(n_steps), int(n_draws)
        ld = (cols + 3) // 4 * 4 if ld is None else int(ld)
        shape = (n_steps, n_draws, rows, ld)
        if out is not None:
            L.require_gpu(out)
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n_steps * n_draws * rows * ld:
                raise ValueError("out must be a contiguous float32 tensor of %d x %d x %d x %d elements, got %s %s"
                                 % (shape + (out.dtype, tuple(out.shape))))
        else:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise L.SocialWaysHipError("DeviceNoise fills on MI355X only: device %s (no CPU fallback)" % dev)
            if min(shape) < 1:
                raise L.SocialWaysHipError("DeviceNoise.fill: empty shape %s" % (shape,))
            out = torch.empty(shape, device=dev)
        for name, v in (("step", step), ("draw0", draw0), ("row0", row0)):
            if not 0 <= int(v) < 1 << 32:
                raise L.SocialWaysHipError("DeviceNoise.fill: %s = %d outside 0 .. 2^32 - 1" % (name, v))
        with torch.cuda.device(out.device):
            L.call("sw_noise_uniform", self.seed, int(domain), int(step), n_steps, int(draw0), n_draws, int(row0), rows, cols, ld,
                   out.data_ptr(), L.stream())
        return out.view(shape)
