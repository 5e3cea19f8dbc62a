"""Training-step harness around the HIP hot path: the ODEConvGRU branch of the reference's
`train_batch` (train_test.py:169-207) and its checkpoint format (helpers/utils.py:212-252), without the per-step host copies
of the reference's loop (train_test.py:50 `pred.detach().cpu()`) and with anomaly detection off (train_test.py:5).  Evaluation
(SURVEY.md section 8 f5): `test_batch` and `evaluate`, the ODEConv branch of the reference's `test_batch` / `test`
(train_test.py:78-165) with the per-frame metrics computed on the device (metrics.py)."""
import os
import pickle

import torch


def train_batch(model, batch_dict, optimizer, async_solver=False, clip=None):
    """One optimisation step.  batch_dict: 'observed_data' (B,T_in,C,H,W) and 'data_to_predict' (B,T_out,C,H,W) in [-0.5, 0.5] as the
    reference's loaders deliver them, plus 'observed_tp' / 'tp_to_predict'.  Returns (pred * 255, truth * 255, loss tensor, loss_dict)
    -- the loss stays on the device (no .item() synchronisation here).

    async_solver (opt-in): a dopri5 solve inside the model only enqueues its attempted steps and the backward pass collects its outcome
    (ode_rl_amd.set_async_dopri5): the host goes on enqueueing decoder, loss and backward while the device still integrates.  A solver
    error (dt underflow, non-finite state) then surfaces at loss.backward(), not inside the forward as in torchdiffeq.  A solve that
    needs more attempted steps than were enqueued up front, or that fails, is SEALED on the device (its unreached frames are NaN, never
    stale memory).  Whatever the asynchronous pass raises, nothing has touched the parameters or the optimiser at that point, and the
    module buffers (BatchNorm statistics, which may have folded in the NaN frames) are restored to their values of before the pass.
    An AsyncSolveTruncated is then handled here: the step is repeated on the synchronous path, whatever the caller's setting (the next
    asynchronous solve enqueues more attempts); any other error is re-raised.  The caller's asynchronous setting is restored
    afterwards, and an error from collecting the solves still pending on the way out never replaces the error of the pass.

    clip: the reference's `opt.clip` (train_test.py:187-195).  None or -1: no clipping, and loss_dict has the keys it always had.
    Otherwise the gradients are clipped to that global L2 norm before the update -- a FusedAdam or FusedAdamax does it inside its step
    (`step(max_grad_norm=clip)`: norm, coefficient and update stay on the device), any other optimizer gets
    torch.nn.utils.clip_grad_norm_ in front of its step() -- and loss_dict['Gradient Norm'] is the norm AFTER clipping as a device
    scalar (the reference logs it from one .item() per parameter tensor).  A batch-sharded loop that all-reduces the gradients itself
    (dist.allreduce_gradients) clips after that: every rank then computes the same coefficient without another collective."""
    dev = next(model.parameters()).device
    inp = batch_dict["observed_data"].to(dev) + 0.5          # train_test.py:180: [-0.5, 0.5] -> [0, 1]
    out = batch_dict["data_to_predict"].to(dev) + 0.5
    from . import _lib, hip_ops

    def step():
        optimizer.zero_grad()   # torch 2 default (set_to_none=True), as train_test.py:176 today: no fill + accumulate kernels per parameter
        pred = model.get_prediction(inp, batch_dict=batch_dict)
        loss = model.get_loss(pred, out)
        loss.backward()
        return pred, loss

    if async_solver:
        # what a sealed pass could leave behind besides gradients (zeroed by the repeat): module buffers -- a BatchNorm behind the
        # solver (VidODE's flow decoder) would fold the NaN frames into its running statistics
        buffers = [(b, b.detach().clone()) for b in model.buffers()]
        was = hip_ops.set_async_dopri5(True)
        try:
            try:
                pred, loss = step()
                hip_ops.collect_pending_solves()   # a solve nobody differentiated through (none in the models here) is checked too
            except BaseException:
                _set_async_quietly(hip_ops, was)   # the pass's error wins over one from collecting what is still pending
                raise
            hip_ops.set_async_dopri5(was)          # (no error so far: one from collecting here is the step's own)
        except BaseException as e:
            with torch.no_grad():
                for b, kept in buffers:
                    b.copy_(kept)
            if not isinstance(e, _lib.AsyncSolveTruncated):
                raise
            hip_ops.set_async_dopri5(False)        # the repeat is synchronous: a second truncation is impossible
            try:
                pred, loss = step()
            finally:
                _set_async_quietly(hip_ops, was)
    else:
        pred, loss = step()
    loss_dict = {"Per Step Loss": loss.detach()}
    if clip is None or clip == -1:
        optimizer.step()
    else:
        from .optim import _FusedOptimizer
        if isinstance(optimizer, _FusedOptimizer):   # FusedAdam, FusedAdamax: the clip is part of their step
            optimizer.step(max_grad_norm=float(clip))
            loss_dict["Gradient Norm"] = optimizer.last_clipped_norm
        else:
            total = torch.nn.utils.clip_grad_norm_(model.parameters(), float(clip))
            optimizer.step()
            loss_dict["Gradient Norm"] = total * torch.clamp(float(clip) / (total + 1e-6), max=1.0)   # the coefficient it applied
    return pred.detach() * 255.0, out * 255.0, loss.detach(), loss_dict


def train_batch_gan(model, netD_img, netD_seq, batch_dict, optimizer_netG, optimizer_netD, lamb_adv=0.003, clip=None):
    """One adversarial step in Vid-ODE's order (Vid-ODE/main.py:221-254) around the `get_prediction` / `get_loss` pair of `train_batch`,
    with the frames in the [0, 1] space `train_batch` works in:
      1. reconstruction loss of the generator `model`;
      2. loss_D = lamb_adv * (netD_seq.netD_adv_loss + netD_img.netD_adv_loss) on the detached prediction;
      3. optimizer_netD.zero_grad(); loss_D.backward(); optimizer_netD.step();
      4. adv = lamb_adv * (netD_seq.netG_adv_loss + netD_img.netG_adv_loss) against the UPDATED discriminators;
      5. optimizer_netG.zero_grad(); (loss + adv).backward(); optimizer_netG.step(), `clip` as in `train_batch`.
    During 4 and 5 the discriminators' parameters have requires_grad switched off (restored afterwards, also when the pass raises): the
    reference computes those gradients and throws them away at its next zero_grad, here their `.grad` stays as step 3 left it.

    Returns (pred * 255, truth * 255, loss, loss_dict); loss is the reconstruction loss, loss_dict carries 'Per Step Loss (netD)' =
    loss_D, 'Per Step Loss (netG)' = adv and 'Per Step Loss' = their sum, as the reference logs them (main.py:265-267) -- device scalars,
    no .item() -- plus 'Gradient Norm' with a clip.

    An irregular batch ('observed_mask' and 'mask_predicted_data' present and not None) gets the reference's frame selection
    (main.py:230-237) by torch indexing before the discriminators see the frames; `int(observed_mask[0].sum())` is one host read, as
    there.  The asynchronous dopri5 option of `train_batch` is not available here."""
    dev = next(model.parameters()).device
    inp = batch_dict["observed_data"].to(dev) + 0.5
    out = batch_dict["data_to_predict"].to(dev) + 0.5
    fake = model.get_prediction(inp, batch_dict=batch_dict)
    loss = model.get_loss(fake, out)
    real, input_real = out, inp
    observed_mask, mask_predicted = batch_dict.get("observed_mask"), batch_dict.get("mask_predicted_data")
    if observed_mask is not None and mask_predicted is not None:
        b, _, c, h, w = real.size()
        n_sel = int(observed_mask[0].sum())
        input_real = input_real[observed_mask.to(dev).squeeze(-1).bool(), ...].view(b, n_sel, c, h, w)
        real = real[mask_predicted.to(dev).squeeze(-1).bool(), ...].view(b, n_sel, c, h, w)

    loss_netD = lamb_adv * netD_seq.netD_adv_loss(real, fake, input_real)
    loss_netD = loss_netD + lamb_adv * netD_img.netD_adv_loss(real, fake, None)
    optimizer_netD.zero_grad()
    loss_netD.backward()
    optimizer_netD.step()

    d_params = [p for net in (netD_img, netD_seq) for p in net.parameters()]
    flags = [p.requires_grad for p in d_params]
    try:
        for p in d_params:
            p.requires_grad_(False)
        loss_adv = lamb_adv * netD_seq.netG_adv_loss(real, fake, input_real)
        loss_adv = loss_adv + lamb_adv * netD_img.netG_adv_loss(None, fake, None)
        optimizer_netG.zero_grad()
        (loss + loss_adv).backward()
    finally:
        for p, flag in zip(d_params, flags):
            p.requires_grad_(flag)
    loss_netD, loss_adv = loss_netD.detach(), loss_adv.detach()
    loss_dict = {"Per Step Loss (netD)": loss_netD, "Per Step Loss (netG)": loss_adv, "Per Step Loss": loss_netD + loss_adv}
    if clip is None or clip == -1:
        optimizer_netG.step()
    else:
        from .optim import _FusedOptimizer
        if isinstance(optimizer_netG, _FusedOptimizer):
            optimizer_netG.step(max_grad_norm=float(clip))
            loss_dict["Gradient Norm"] = optimizer_netG.last_clipped_norm
        else:
            total = torch.nn.utils.clip_grad_norm_(model.parameters(), float(clip))
            optimizer_netG.step()
            loss_dict["Gradient Norm"] = total * torch.clamp(float(clip) / (total + 1e-6), max=1.0)
    return fake.detach() * 255.0, out * 255.0, loss.detach(), loss_dict


def _set_async_quietly(hip_ops, on):
    """set_async_dopri5(on) while another exception is in flight: switching off collects the pending solves, and an error of theirs
    is dropped so that it cannot replace the one being raised (the switch is set before the collection, so it holds either way)."""
    try:
        hip_ops.set_async_dopri5(on)
    except Exception:
        pass


def test_batch(model, batch_dict):
    """The ODEConv branch of the reference's `test_batch` (train_test.py:146-167) for one batch as `data.get_next_batch` builds it:
    frames in [-0.5, 0.5] are shifted to [0, 1] for the model and its loss and back for the result.  Returns (pred - 0.5,
    truth - 0.5, loss) with the loss left on the device.  Gradient mode and model.eval() are the caller's business (`evaluate`)."""
    dev = next(model.parameters()).device
    inp = batch_dict["observed_data"].to(dev) + 0.5
    truth = batch_dict["data_to_predict"].to(dev) + 0.5
    pred = model.get_prediction(inp, batch_dict=batch_dict)
    loss = model.get_loss(pred, truth)
    return pred - 0.5, truth - 0.5, loss


def evaluate(model, batches):
    """The reference's `test()` loop (train_test.py:78-144) without wandb, prints and the video: model.eval() under no_grad, and per
    batch `test_batch`, then MSE, PSNR and SSIM of every predicted frame from ONE `frame_metrics` call where the reference runs
    `F.mse_loss(...).item()`, `math.log10` and `utils.get_normalized_ssim` (a host copy and B scikit-image calls) per frame.  The
    frames go to it in [0, 1] with data_range 1: that is the reference's SSIM of the x 255 frames with data_range 255, and its MSE
    of the [-0.5, 0.5] frames (a shift cancels in the difference), so its `10 log10(1 / mse)` too.  Everything accumulates on the
    device; the single host transfer is at the end.  `batches`: an iterable of batch dicts, at least one.

    Returns a dict: 'mse', 'psnr', 'ssim' -- (T_out,) CPU tensors, the means over the batches per predicted frame (PSNR is the mean
    of the per-batch PSNRs, as the reference averages them, not the PSNR of the mean MSE) -- 'loss' (mean over the batches, a
    float) and 'avg_mse', 'avg_psnr', 'avg_ssim': the last frame's values, which the reference logs as its final metrics
    (train_test.py:143).  The model's training mode is restored on the way out, also when a batch raises."""
    from . import metrics
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            total, loss_sum, n = None, None, 0
            for batch_dict in batches:
                pred, truth, loss = test_batch(model, batch_dict)
                m = metrics.frame_metrics(pred + 0.5, truth + 0.5, data_range=1.0)
                per_frame = torch.stack([m.mse, m.psnr, m.ssim])
                total = per_frame if total is None else total + per_frame
                loss_sum = loss if loss_sum is None else loss_sum + loss
                n += 1
            if n == 0:
                raise ValueError("evaluate: no batches")
            host = torch.cat([(total / n).reshape(-1), torch.as_tensor(loss_sum / n, dtype=total.dtype, device=total.device).reshape(1)]).cpu()
    finally:
        model.train(was_training)
    mse, psnr, ssim = host[:-1].view(3, -1)
    return {"mse": mse, "psnr": psnr, "ssim": ssim, "loss": float(host[-1]),
            "avg_mse": float(mse[-1]), "avg_psnr": float(psnr[-1]), "avg_ssim": float(ssim[-1])}


def _select_frames(frames, mask):
    """Upstream's `data[mask.squeeze(-1).byte()].view(b, int(mask[0].sum()), c, h, w)` (Vid-ODE/tester.py:65-67) without a device
    read: the mask is looked at where the loader left it (the host), a mask that keeps every frame selects nothing, and the others
    index with positions uploaded through pinned memory.  mask: None, (B, T, 1) or (B, T)."""
    import numpy as np
    from . import vidode_data
    if mask is None:
        return frames
    b, t = frames.shape[:2]
    keep = mask.detach().cpu().reshape(b, -1).numpy() != 0
    if keep.shape[1] != t:
        raise ValueError(f"evaluate_vidode: mask_predicted_data {tuple(mask.shape)} does not match the {t} frames of data_to_predict")
    if keep.all():
        return frames
    n = int(keep[0].sum())
    if not (keep.sum(axis=1) == n).all():
        raise ValueError(f"evaluate_vidode: mask_predicted_data keeps {keep.sum(axis=1).tolist()} frames per sample; upstream's view needs "
                         "the same number in every sample")
    cols = torch.from_numpy(np.stack([np.nonzero(row)[0] for row in keep]).reshape(b, n))
    rows = torch.arange(b).unsqueeze(-1).expand_as(cols).contiguous()
    return frames[vidode_data._upload(rows, frames.device), vidode_data._upload(cols, frames.device)]


def evaluate_vidode(model, loader, opt, n_batches=None):
    """Upstream Vid-ODE's `Tester.infer_and_metrics` (Vid-ODE/tester.py:49-78) with `visualize.save_test_images` and
    `evaluate.Evaluation` behind it, without the PNG files: model.eval() under no_grad, and per batch of `loader` (the dictionaries a
    `vidode_data.VidODEBatches` yields) `vidode_data.get_next_batch(..., test_interp=not opt.extrap)`, `model.get_reconstruction` with
    upstream's five arguments, `data_to_predict` selected by `mask_predicted_data`, then `PngEvaluation.update(preds, truth,
    input_norm=opt.input_norm)`: 8-bit RGB bytes, luma SSIM and byte MSE accumulated on the device.  `n_batches` ends an endless loader
    (upstream's `n_test_batches`); a finite iterable needs none.

    Returns {'ssim', 'mse', 'psnr', 'n_images'}: upstream's avg_ssim, avg_mse and avg_psnr = 10 log10(1 / avg_mse) over all images, from
    the one host transfer at the end.  Left out: writing the PNG files, `os.listdir`, and upstream's `rm -rf` of the result directory.
    The model's training mode is restored on the way out, also when a batch raises."""
    from . import metrics, vidode_data
    if getattr(opt, "dataset", None) == "hurricane":
        raise NotImplementedError("evaluate_vidode: the Hurricane set is not implemented (its loader needs Pad and ToTensor(scale=False), "
                                  "and upstream scores its 'orignal_data_to_predict')")
    test_interp = not opt.extrap
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            ev, seen = None, 0
            for data_dict in loader:
                if n_batches is not None and seen >= n_batches:
                    break
                batch_dict = vidode_data.get_next_batch(data_dict, test_interp=test_interp)
                preds, _ = model.get_reconstruction(time_steps_to_predict=batch_dict["tp_to_predict"], truth=batch_dict["observed_data"],
                                                    truth_time_steps=batch_dict["observed_tp"], mask=batch_dict["observed_mask"],
                                                    out_mask=batch_dict["mask_predicted_data"])
                truth = _select_frames(batch_dict["data_to_predict"].to(preds.device), batch_dict["mask_predicted_data"])
                if ev is None:
                    ev = metrics.PngEvaluation(preds.device)
                ev.update(preds, truth, input_norm=bool(getattr(opt, "input_norm", False)))
                seen += 1
            if ev is None:
                raise ValueError("evaluate_vidode: no batches")
            avg_ssim, avg_mse, avg_psnr, n_images = ev.summary()
    finally:
        model.train(was_training)
    return {"ssim": avg_ssim, "mse": avg_mse, "psnr": avg_psnr, "n_images": n_images}


def checkpoint_name(ckpt_id, step):
    return f"{ckpt_id}_{step:010d}.pickle"                    # helpers/utils.py:215-217


def save_model_params(model, optimizer, epoch, step, logdir, ckpt_id):
    """Same pickle as helpers/utils.py:212-226: {'epoch', 'step', 'state_dict', 'optimizer'} (aliased state_dict keys kept)."""
    path = os.path.join(logdir, checkpoint_name(ckpt_id, step))
    blob = {"epoch": epoch, "step": step,
            "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
            "optimizer": optimizer.state_dict()}
    with open(path, "wb") as fh:
        pickle.dump(blob, fh, protocol=pickle.HIGHEST_PROTOCOL)
    return path


def load_model_params(model, path, optimizer=None):
    with open(path, "rb") as fh:
        blob = pickle.load(fh)
    model.load_state_dict(blob["state_dict"])
    if optimizer is not None and "optimizer" in blob:
        optimizer.load_state_dict(blob["optimizer"])
    return blob.get("epoch"), blob.get("step")
