"""In-batch cross-modal InfoNCE (the symmetric CLIP / GDT-style loss) on the gfx950 kernel ``avid_infonce``: the other
modality's embeddings of the global batch are the negatives — no memory bank, no sampler, no partition constant."""
import torch
from torch import nn
import torch.distributed as dist

from avid_hip import ops
from avid_hip.lib import AvidHipError
from utils.distributed_utils import _gather_from_all

__all__ = ['InfoNCE']


def gather_embeddings(v_hat, a_hat):
    """Both modalities' unit-norm embeddings of every rank in ONE all_gather: a packed [b, 2D] record per sample (as
    ``criterions.avid.gather_update_records`` packs its records).  Returns (v_all, a_all, row0) — the gathered copies carry
    no gradient; rows [row0, row0 + b) are this rank's."""
    b, D = v_hat.shape
    rec = torch.empty((b, 2 * D), dtype=torch.float32, device=v_hat.device)
    with torch.no_grad():
        rec[:, :D] = v_hat
        rec[:, D:] = a_hat
        allrec = _gather_from_all(rec)
    return allrec[:, :D].contiguous(), allrec[:, D:].contiguous(), dist.get_rank() * b


class InfoNCE(nn.Module):
    """``forward(emb1, emb2, target) -> (loss, tb_log)`` like ``AVID``; ``target`` (the sample ids) is not used.

    loss = v2a_coeff * CE(v -> a) + a2v_coeff * CE(a -> v) over the GLOBAL batch, coefficients normalised to sum to 1,
    scores = cosine / temperature.  Under an initialised process group of R > 1 ranks every rank gathers all embeddings,
    returns the same global loss and back-propagates R times the exact gradient of that loss for its own rows — the
    engines and DistributedDataParallel average gradients with 1 / R, which leaves exactly the gradient of the global loss.
    ``num_data`` and the memory bank's own arguments (``num_negatives``, ``momentum``, ``xModal_coeff``, ``wModal_coeff``,
    ``checkpoint``) are accepted and ignored so that a configuration written for ``AVID`` runs with only ``loss.name`` swapped;
    any other keyword is a TypeError.  No parameters, no buffers: the state dict is empty."""

    BANK_ARGS = ("num_negatives", "momentum", "xModal_coeff", "wModal_coeff", "checkpoint")

    in_batch_negatives = True    # avid_hip.parallel.TrainStep: a shard-after-shard (virtual_ranks > 1) step is refused

    def __init__(self, embedding_dim, device=0, temperature=0.07, v2a_coeff=1., a2v_coeff=1., num_data=None,
                 **bank_args):
        super(InfoNCE, self).__init__()
        unknown = sorted(set(bank_args) - set(self.BANK_ARGS))
        if unknown:
            raise TypeError(f"InfoNCE.__init__() got unexpected keyword argument(s) {unknown}")
        embedding_dim, temperature = int(embedding_dim), float(temperature)
        if embedding_dim % 32 or not 32 <= embedding_dim <= 512:
            raise ValueError(f"InfoNCE: embedding_dim = {embedding_dim}: a multiple of 32 up to 512 expected")
        if not 0. < temperature < float('inf'):
            raise ValueError(f"InfoNCE: temperature = {temperature!r} must be positive and finite")
        v2a_coeff, a2v_coeff = float(v2a_coeff), float(a2v_coeff)
        if not (v2a_coeff >= 0. and a2v_coeff >= 0. and 0. < v2a_coeff + a2v_coeff < float('inf')):
            raise ValueError(f"InfoNCE: coefficients ({v2a_coeff!r}, {a2v_coeff!r}) must be >= 0 with a positive finite sum")
        self.embedding_dim = embedding_dim
        self.temperature = temperature
        self.v2a_coeff = v2a_coeff / (v2a_coeff + a2v_coeff)
        self.a2v_coeff = a2v_coeff / (v2a_coeff + a2v_coeff)
        self.device = device
        self._ws, self._ws_key = None, None

    def _check(self, emb1, emb2):
        for name, t in (("emb1", emb1), ("emb2", emb2)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise AvidHipError(f"InfoNCE: {name} must be a HIP device tensor — there is no CPU fallback")
            if t.dtype != torch.float32:
                raise AvidHipError(f"InfoNCE: {name} must be float32, got {t.dtype}")
        if emb1.dim() != 2 or tuple(emb1.shape) != tuple(emb2.shape) or emb1.shape[0] < 1 or emb1.device != emb2.device:
            raise AvidHipError(f"InfoNCE: embeddings {tuple(emb1.shape)} and {tuple(emb2.shape)} must be [b, D] on one device")
        if emb1.shape[1] != self.embedding_dim:
            raise AvidHipError(f"InfoNCE: embedding width {emb1.shape[1]}, the criterion was built for {self.embedding_dim}")

    def forward(self, emb1, emb2, target=None):
        self._check(emb1, emb2)
        v_hat = ops.l2_normalize(emb1)
        a_hat = ops.l2_normalize(emb2)
        b = v_hat.shape[0]
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        row0 = 0
        if world > 1:
            v_all, a_all, row0 = gather_embeddings(v_hat, a_hat)
            # the local rows enter as themselves (same bits as their gathered copies) so that their gradient reaches the towers
            v_hat = torch.cat([v_all[:row0], v_hat, v_all[row0 + b:]])
            a_hat = torch.cat([a_all[:row0], a_hat, a_all[row0 + b:]])
        G = v_hat.shape[0]
        key = (G, v_hat.device)
        if self._ws_key != key:
            self._ws, self._ws_key = ops.infonce_workspace(v_hat.device, G), key
        loss, losses, hits, _ = ops.infonce(v_hat, a_hat, row0=row0, b=b, inv_T=1.0 / self.temperature,
                                            weights=(self.v2a_coeff, self.a2v_coeff), grad_scale=float(world), ws=self._ws)
        acc = hits.to(torch.float32) * (100.0 / G)
        tb_log = {'Loss/v2a': losses[1], 'Loss/a2v': losses[2], 'Acc/v2a': acc[0], 'Acc/a2v': acc[1]}
        return loss, tb_log

    def set_epoch(self, epoch):
        pass

    def extra_repr(self):
        return (f"embedding_dim={self.embedding_dim}, temperature={self.temperature}, v2a_coeff={self.v2a_coeff}, "
                f"a2v_coeff={self.a2v_coeff}")
