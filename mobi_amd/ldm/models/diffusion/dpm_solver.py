"""DPM-Solver++(2M) sampler on the engine (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
Probabilistic Models", 2022: the multistep second-order solver in data prediction form), under the name and call
signature Stable Diffusion's `ldm.models.diffusion.dpm_solver.DPMSolverSampler` users expect.

Grid: the DDIM grid, so that DPM-S and DDIM-S start and end at the same points -- make_ddim_timesteps("uniform", S)
descending, then one end point with abar = alphas_cumprod[0] (the a_prev of DDIM's last step).  At every grid point
alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log alpha - log sigma; step i goes from s = grid[i] to
t = grid[i + 1] with h_i = lambda_t - lambda_s:
  x0_i = (x - sigma_s eps) / alpha_s
  first order (step 0; the last step too when S < 15):  x_t = sigma_t/sigma_s x - alpha_t (e^-h - 1) x0_i
  second order, r = h_{i-1} / h_i:  D = (1 + 1/(2r)) x0_i - 1/(2r) x0_{i-1};  x_t = sigma_t/sigma_s x - alpha_t (e^-h - 1) D
The per-step coefficients are computed in fp64 on the host and rounded once to fp32 (`dpm_coefficients`); the update is
one HIP kernel (mobi_dpm_step, fp32, order in include/mobi_engine.h).  The first-order map is DDIM with eta = 0.
On the GPU a step is ONE graph launch (mobi_amd/graph.py, kind "dpm"): UNet evaluation(s) plus the update, reading its
coefficient row and the x0 history from device buffers, so one capture serves every step of a run."""
import numpy as np
import torch

from .... import graph, ops
from ...modules.diffusionmodules.util import make_ddim_timesteps
from .ddim import DDIMSampler

# S below this: the last step is first order (DPM-Solver's `lower_order_final`, which keeps few-step runs stable).  S is
# the requested step count: make_ddim_timesteps may return one point more (S = 14 gives 15)
LOWER_ORDER_FINAL_BELOW = 15


def dpm_grid(alphas_cumprod, S, num_timesteps):
    """(timesteps [n] int64 descending, abar [n + 1] fp64): the DDIM grid of S steps, then abar = alphas_cumprod[0]."""
    ac = alphas_cumprod.detach().cpu().numpy() if isinstance(alphas_cumprod, torch.Tensor) else alphas_cumprod
    ac = np.asarray(ac, dtype=np.float64)
    ts = np.flip(make_ddim_timesteps("uniform", S, num_timesteps, verbose=False)).copy()
    return ts, np.concatenate([ac[ts], ac[:1]])


def dpm_coefficients(abar, final_first_order):
    """fp64 [n, 5] = {1/alpha_s, sigma_s/alpha_s, c_x, c_0, c_1} per step of the grid `abar` ([n + 1]); x_t =
    c_x x + c_0 x0_i + c_1 x0_{i-1}.  Step 0 (and the last step when `final_first_order`) is first order: c_1 = 0."""
    abar = np.asarray(abar, dtype=np.float64)
    n = abar.shape[0] - 1
    alpha, sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
    lam = np.log(alpha) - np.log(sigma)
    h = lam[1:] - lam[:-1]
    tab = np.zeros((n, 5), dtype=np.float64)
    for i in range(n):
        phi = np.exp(-h[i]) - 1.0
        tab[i, 0], tab[i, 1], tab[i, 2] = 1.0 / alpha[i], sigma[i] / alpha[i], sigma[i + 1] / sigma[i]
        if i == 0 or (i == n - 1 and final_first_order):
            tab[i, 3] = -alpha[i + 1] * phi
        else:
            k = 1.0 / (2.0 * (h[i - 1] / h[i]))
            tab[i, 3] = -alpha[i + 1] * phi * (1.0 + k)
            tab[i, 4] = alpha[i + 1] * phi * k
    return tab


class DPMSolverSampler(object):
    def __init__(self, model, graph=True, **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.use_graph = bool(graph)              # one HIP graph launch per step (mobi_amd/graph.py)

    # the UNet evaluation(s) of a step -> (e_cond, e_uncond | None); the classifier-free mix happens in mobi_dpm_step
    _eps = DDIMSampler._eps

    def make_schedule(self, S, verbose=True):
        self.ddim_timesteps = make_ddim_timesteps("uniform", S, self.ddpm_num_timesteps, verbose=verbose)
        self.timesteps, self.abar = dpm_grid(self.model.alphas_cumprod, S, self.ddpm_num_timesteps)
        self.coef = dpm_coefficients(self.abar, S < LOWER_ORDER_FINAL_BELOW).astype(np.float32)
        self._coef_dev = torch.from_numpy(self.coef).to(self.model.betas.device)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., x_T=None, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, callback=None, img_callback=None, log_every_t=100, verbose=True,
               mask=None, x0=None, quantize_x0=False, score_corrector=None, noise_dropout=0., inpaint_image=None,
               inpaint_mask=None, **kwargs):
        if eta != 0:
            raise ValueError("eta must be 0 for DPM-Solver++(2M): it is an ODE solver")
        if mask is not None or x0 is not None:
            raise NotImplementedError("mask / x0 blending is not on the DPM-Solver path")
        if quantize_x0 or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError("quantize_x0 / score_corrector / noise_dropout are not on MObI's path")
        if "test_model_kwargs" in kwargs:          # the reference harness's DDIM spelling
            kw = {"test_model_kwargs": kwargs["test_model_kwargs"]}
        elif "rest" in kwargs:
            kw = {"rest": kwargs["rest"]}
        elif inpaint_image is not None and inpaint_mask is not None:      # its PLMS spelling
            kw = {"test_model_kwargs": {"inpaint_image": inpaint_image, "inpaint_mask": inpaint_mask}}
        else:
            raise Exception("kwargs must contain either 'test_model_kwargs' or 'rest' key, or inpaint_image / inpaint_mask")
        self.make_schedule(S, verbose=verbose)
        C, H, W = shape
        return self.dpm_sampling(conditioning, (batch_size, C, H, W), kw, x_T=x_T,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning, callback=callback,
                                 img_callback=img_callback, log_every_t=log_every_t)

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, kw, x_T=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                     callback=None, img_callback=None, log_every_t=100):
        device = self.model.betas.device
        b = shape[0]
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        img = img.contiguous()
        scale, uc = unconditional_guidance_scale, unconditional_conditioning
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        total_steps = self.timesteps.shape[0]
        self._weights_fp = graph.weights_fingerprint(self.model)
        graphed = self.use_graph and graph.usable(img) and isinstance(cond, torch.Tensor)
        keep = (lambda t_: t_.clone()) if graphed else (lambda t_: t_)     # graph outputs are overwritten next step
        x0_hist = None if graphed else torch.empty_like(img)             # the eager path's history (step 0 never reads it)
        for i, step in enumerate(self.timesteps):
            if graphed:
                g = graph.get(self, "dpm", img, cond, uc, scale, kw)
                img, pred_x0 = g.run(img, int(step), self._coef_dev[i])
            else:
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                e_cond, e_uncond = self._eps(img, cond, ts, scale, uc, kw)
                c = [float(v) for v in self.coef[i]]
                img, pred_x0 = ops.dpm_step(img, e_cond, x0_hist, e_uncond=e_uncond, cfg_scale=float(scale),
                                            inv_alpha_s=c[0], sigma_over_alpha_s=c[1], c_x=c[2], c_0=c[3], c_1=c[4])
            if callback:
                callback(i)
            if img_callback:
                img_callback(keep(pred_x0), i)
            index = total_steps - i - 1
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["x_inter"].append(keep(img))
                intermediates["pred_x0"].append(keep(pred_x0))
        return keep(img), intermediates
