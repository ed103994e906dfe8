"""Flow-matching Euler schedule (host mirror of the diffusers object the reference passes around).

The reference reaches ``scheduler.sigmas`` / ``index_for_timestep`` / ``set_timesteps`` at
adv_grpo/diffusers_patch/sd3_sde_with_logprob.py:106-110 and
sd3_pipeline_with_logprob_fast.py:574; SD3.5-medium config: 1000 train steps, shift 3.0, static
shift applied on the inference grid as well.  Unlike the reference's per-sample
``(timesteps == t).nonzero().item()`` (one host sync per sample per step) the index is resolved
on the host copy of the schedule; only the 11-float sigma table lives on the device.
"""
import threading

import numpy as np
import torch


class FlowMatchEulerDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, shift=3.0, device=None):
        self.num_train_timesteps = num_train_timesteps
        self.shift = shift
        self.device = device
        sig = np.linspace(1, num_train_timesteps, num_train_timesteps, dtype=np.float32)[::-1] / np.float32(
            num_train_timesteps)
        sig = (np.float32(shift) * sig / (1 + (np.float32(shift) - 1) * sig)).astype(np.float32)
        self.sigma_max = float(sig[0])
        self.sigma_min = float(sig[-1])
        self._lock = threading.Lock()    # first fill of a table: two rollout threads may miss at the same time
        self._tables = {}          # (n_steps, device) -> (sigmas_host, timesteps_host, sigmas, timesteps): immutable, never freed
        self._install(sig, append_zero=False)

    def _install(self, sig, append_zero):
        sig = np.asarray(sig, dtype=np.float32)
        ts = sig * np.float32(self.num_train_timesteps)
        if append_zero:
            sig = np.concatenate([sig, np.zeros(1, dtype=np.float32)])
        self._sigmas_host = sig
        self._timesteps_host = ts
        self.sigmas = torch.from_numpy(sig.copy()).to(self.device) if self.device else torch.from_numpy(sig.copy())
        self.timesteps = torch.from_numpy(ts.copy()).to(self.device) if self.device else torch.from_numpy(ts.copy())

    def set_timesteps(self, num_inference_steps, device=None):
        """Installs the n-step table.  The device tensors of a given (n, device) are built ONCE and kept for the life of the
        scheduler: concurrent rollouts (two prompt groups in flight on two streams, trainer.sample_epoch) each re-install the
        same objects, so no kernel queued on another stream can find its sigma table freed and recycled under it."""
        if device is not None:
            self.device = device
        key = (int(num_inference_steps), str(self.device))
        hit = self._tables.get(key)
        if hit is not None:
            self._sigmas_host, self._timesteps_host, self.sigmas, self.timesteps = hit
            return
        with self._lock:
            self._build(key, num_inference_steps)

    def _build(self, key, num_inference_steps):
        hit = self._tables.get(key)         # (filled by the thread that held the lock before us)
        if hit is not None:
            self._sigmas_host, self._timesteps_host, self.sigmas, self.timesteps = hit
            return
        t = np.linspace(self.sigma_max * self.num_train_timesteps, self.sigma_min * self.num_train_timesteps,
                        num_inference_steps)
        sig = t / self.num_train_timesteps
        sig = self.shift * sig / (1 + (self.shift - 1) * sig)
        self._install(sig.astype(np.float32), append_zero=True)
        if self.sigmas.is_cuda:
            torch.cuda.current_stream(self.sigmas.device).synchronize()     # one-time: the tables are complete before any stream reads them
        self._tables[key] = (self._sigmas_host, self._timesteps_host, self.sigmas, self.timesteps)

    def index_for_timestep(self, timestep):
        t = float(timestep)
        hits = np.nonzero(self._timesteps_host == np.float32(t))[0]
        if len(hits) == 0:
            raise ValueError(f"timestep {t} is not on the schedule")
        return int(hits[1] if len(hits) > 1 else hits[0])


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, **kwargs):
    scheduler.set_timesteps(num_inference_steps, device=device)
    return scheduler.timesteps, num_inference_steps


def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=8192, base_shift=0.5, max_shift=0.9):
    """QwenImagePipeline's ``calculate_shift``: mu, linear in the number of image tokens."""
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


class QwenImageFlowMatchScheduler:
    """The configuration of diffusers' ``FlowMatchEulerDiscreteScheduler`` that Qwen-Image ships (scheduler/scheduler_config.json:
    use_dynamic_shifting, exponential time shift, shift_terminal 0.02) as ``QwenImagePipeline.__call__`` drives it: PARITY UNPINNED,
    restated from the published code (scripts/verify_against_diffusers.py compares where diffusers is installed).

        raw    = linspace(1, 1/n, n)
        s      = exp(mu) / (exp(mu) + (1/raw - 1))          mu = calculate_shift(N_img): the table depends on the image size
        sigmas = 1 - (1 - s) / ((1 - s[-1]) / (1 - shift_terminal)) ; timesteps = 1000 * sigmas ; then 0 is appended to sigmas

    Deviation: diffusers evaluates this chain in float32 numpy; here it runs in float64 and is rounded to float32 once, so the table
    is the correctly rounded one (sigmas[0] == 1 and sigmas[n-1] == shift_terminal to f32 rounding).  The two differ by a few f32 ulp of 1.
    A sibling of the SD3 class above, which it leaves alone; device tables are built once per (n, N_img, device) and never freed."""
    order = 1

    def __init__(self, num_train_timesteps=1000, base_image_seq_len=256, max_image_seq_len=8192, base_shift=0.5, max_shift=0.9,
                 shift_terminal=0.02, device=None):
        self.num_train_timesteps = num_train_timesteps
        self.base_image_seq_len, self.max_image_seq_len = base_image_seq_len, max_image_seq_len
        self.base_shift, self.max_shift, self.shift_terminal = base_shift, max_shift, shift_terminal
        self.device = device
        self._lock = threading.Lock()
        self._tables = {}          # (n_steps, N_img, device) -> (sigmas_host, timesteps_host, sigmas, timesteps)
        self.sigmas = self.timesteps = self._sigmas_host = self._timesteps_host = None

    def mu(self, image_seq_len):
        return calculate_shift(image_seq_len, self.base_image_seq_len, self.max_image_seq_len, self.base_shift, self.max_shift)

    def table(self, num_inference_steps, image_seq_len):
        """-> (sigmas [n + 1], timesteps [n]) float32 numpy."""
        n = int(num_inference_steps)
        raw = np.linspace(1.0, 1.0 / n, n, dtype=np.float64)
        e = np.exp(np.float64(self.mu(image_seq_len)))
        s = e / (e + (1.0 / raw - 1.0))
        if self.shift_terminal:
            s = 1.0 - (1.0 - s) / ((1.0 - s[-1]) / (1.0 - self.shift_terminal))
        sig = s.astype(np.float32)
        ts = sig * np.float32(self.num_train_timesteps)
        return np.concatenate([sig, np.zeros(1, dtype=np.float32)]), ts

    def set_timesteps(self, num_inference_steps, image_seq_len, device=None):
        if device is not None:
            self.device = device
        key = (int(num_inference_steps), int(image_seq_len), str(self.device))
        with self._lock:
            hit = self._tables.get(key)
            if hit is None:
                sig, ts = self.table(num_inference_steps, image_seq_len)
                dev = self.device if self.device else "cpu"
                hit = (sig, ts, torch.from_numpy(sig.copy()).to(dev), torch.from_numpy(ts.copy()).to(dev))
                if hit[2].is_cuda:
                    torch.cuda.current_stream(hit[2].device).synchronize()     # one-time: complete before any stream reads them
                self._tables[key] = hit
            self._sigmas_host, self._timesteps_host, self.sigmas, self.timesteps = hit
        return self.timesteps
