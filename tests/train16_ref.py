"""CPU reference for the mixed-precision training step (plain helper module like
linear16_ref.py, no GPU needed).

train_step(): one fp64 training iteration of a deep copy of an oracle.OracleDLRM in which
every Linear below the head computes, with r16 = the fp32 value rounded to nearest-even
``dt``:
    forward   y  = r16(x) r16(W)^T + b
    backward  gx = r16(g) r16(W),  gW = r16(g)^T r16(x),  gb = sum_m r16(g)
(one rounded copy of g - the gradient at the Linear's output, after the ReLU mask - for all
three, as the device's dgrad and wgrad launches both round the same g).  The head's K -> 1
layer, the biases, the activations, the lookup, the interaction, the loss and the update
stay unrounded.  dt=None rounds nothing: the step is then OracleDLRM.train_step in fp64."""
import copy

import torch

import oracle as O  # noqa: F401  (the models this module steps)
from linear16_ref import r16


class Linear16(torch.autograd.Function):
    """y = r16(x) r16(W)^T + b with the rounded backward above (dt None: plain Linear)."""

    @staticmethod
    def forward(ctx, x, W, b, dt):
        xr, Wr = r16(x, dt), r16(W, dt)
        ctx.save_for_backward(xr, Wr)
        ctx.dt = dt
        return xr @ Wr.t() + b

    @staticmethod
    def backward(ctx, g):
        xr, Wr = ctx.saved_tensors
        gr = r16(g, ctx.dt)
        return gr @ Wr, gr.t() @ xr, gr.sum(0), None


def linear16_grads(x, W, g, dt):
    """(gx, gW, gb) of one rounded Linear for an output gradient g (fp64 tensors)."""
    gr, xr, Wr = r16(g, dt), r16(x, dt), r16(W, dt)
    return gr @ Wr, gr.t() @ xr, gr.sum(0)


def clone64(ref):
    """An fp64 deep copy of an OracleDLRM (the caller's model is never touched)."""
    return copy.deepcopy(ref).double()


def _mlp(seq, h, dt, head):
    mods = list(seq)
    linears = [m for m in mods if isinstance(m, torch.nn.Linear)]
    for m in mods:
        if isinstance(m, torch.nn.Linear):
            rounded = None if (head and m is linears[-1]) else dt
            h = Linear16.apply(h, m.weight, m.bias, rounded)
        else:
            h = m(h)
    return h


def forward(model, X, lS_o, lS_i, dt=None):
    """prob [B, 1] (fp64, with autograd history) of the fp64 model."""
    x = _mlp(model.bot_l, torch.as_tensor(X).double(), dt, False)
    ly = model.apply_emb(torch.as_tensor(lS_o), [torch.as_tensor(i) for i in lS_i])
    z = O.interact(x, ly, model.op, model.itself)
    p = _mlp(model.top_l, z, dt, True)
    if 0.0 < model.loss_threshold < 1.0:
        p = torch.clamp(p, min=model.loss_threshold, max=1.0 - model.loss_threshold)
    return p


def train_step(model, X, lS_o, lS_i, T, lr, dt=None, opt=None):
    """One iteration IN PLACE on ``model`` (from clone64): SGD with ``lr``, or ``opt.step()``
    when an optimizer over model.parameters() is given (oracle.RWSAdagradOracle).  Returns
    (prob [B], loss) as fp64 numpy / float, computed before the update."""
    Z = forward(model, X, lS_o, lS_i, dt)
    E = model.loss_fn(Z, torch.as_tensor(T).double().reshape(Z.shape))
    for p in model.parameters():
        p.grad = None
    E.backward()
    if opt is not None:
        opt.step()
    else:
        with torch.no_grad():
            for p in model.parameters():
                if p.grad is not None:
                    p.add_(p.grad, alpha=-lr)
    return Z.detach().numpy().ravel(), float(E.detach())


def predict(model, X, lS_o, lS_i, dt=None):
    with torch.no_grad():
        return forward(model, X, lS_o, lS_i, dt).numpy().ravel()
