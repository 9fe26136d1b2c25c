"""Multi-GPU sampling: independent utterances sharded over ranks, one all-gather to collate.

The reference pins inference to one GPU (convofusion/config.py:92-95).  Utterances are independent
(SURVEY.md section 8e), so each rank (one process per GPU) samples its own slice with its own Philox
sub-stream (``first_utterance`` = global id of its first utterance, so results do not depend on the
number of GPUs) and the final latents are collated with ONE ``all_gather`` (RCCL over xGMI on MI355X;
gloo in the CPU tests).  There is no per-step communication.
"""
import torch
import torch.distributed as dist


def shard_range(total, rank, world_size):
    """Contiguous [start, stop) slice of ``total`` utterances owned by ``rank`` (sizes differ by <= 1)."""
    base, rem = divmod(total, world_size)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def shard_cfg_batch(t, start, stop, total, chunks=7):
    """Slice utterances [start, stop) out of a chunk-major guidance batch [chunks*total, ...]."""
    if t is None:
        return None
    v = t.reshape(chunks, total, *t.shape[1:])
    return v[:, start:stop].reshape(chunks * (stop - start), *t.shape[1:]).contiguous()


def gather_latents(local, total, group=None):
    """all_gather of per-rank latents [b_r, L, 128] -> [total, L, 128] (ragged shards are padded)."""
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return local
    ws = dist.get_world_size(group)
    sizes = [shard_range(total, r, ws) for r in range(ws)]
    mx = max(b - a for a, b in sizes)
    pad = local
    if local.shape[0] < mx:
        pad = torch.cat([local, local.new_zeros((mx - local.shape[0],) + tuple(local.shape[1:]))], dim=0)
    out = [torch.empty_like(pad) for _ in range(ws)]
    dist.all_gather(out, pad.contiguous(), group=group)
    return torch.cat([o[: b - a] for o, (a, b) in zip(out, sizes)], dim=0)


def shard_modality_weights(modality_weights, start, stop, total):
    """The utterances [start, stop) of per-modality guidance weights (``sampler.check_modality_weights``): a dict, a [6] row and an
    [N, 1, 6] table apply to every utterance and are returned as they are; [total, 6] and [N, total, 6] are sliced on the utterance axis."""
    if modality_weights is None or isinstance(modality_weights, dict):
        return modality_weights
    shape = tuple(modality_weights.shape)
    if len(shape) == 2:
        if shape[0] != total:
            raise ValueError(f"modality_weights [B, 6] has {shape[0]} rows for {total} utterances")
        return modality_weights[start:stop]
    if len(shape) == 3 and shape[1] != 1:
        if shape[1] != total:
            raise ValueError(f"modality_weights [N, B, 6] has {shape[1]} utterances, the batch {total}")
        return modality_weights[:, start:stop]
    return modality_weights


def shard_tie(tie, start, stop, total):
    """The rows [start, stop) of a tie table [total, L] (``sampler.check_tie``) for a rank that runs those rows alone, renumbered to the
    slice (entry v >= 0 becomes v - start * L).  Ties cross rows and shards do not talk: a tied token of the slice whose source lies in
    another rank's rows raises ValueError."""
    if tuple(tie.shape[:1]) != (total,) or tie.dim() != 2:
        raise ValueError(f"tie has shape {list(tie.shape)} for {total} utterances: it must be [total, L]")
    L = int(tie.shape[1])
    local = tie[start:stop].to(torch.int64)
    tied = local >= 0
    outside = tied & ((local < start * L) | (local >= stop * L))
    if bool(outside.any()):
        b, l = (int(v) for v in torch.nonzero(outside)[0])
        raise ValueError(f"tie[{start + b}][{l}] = {int(local[b, l])} crosses this rank's rows [{start}, {stop}): a tie must stay inside one "
                         "rank's slice (shards do not communicate)")
    return torch.where(tied, local - start * L, local).to(tie.dtype)


def shard_noise_space(noise_space, start, stop, total):
    """The utterances [start, stop) of a noise space (trajectory [N + 1, total, L, 128], noise [N, total, L, 128]): both rings sliced on
    the utterance axis, contiguous."""
    trajectory, noise = noise_space
    for name, t in (("trajectory", trajectory), ("noise", noise)):
        if t.dim() != 4 or t.shape[1] != total:
            raise ValueError(f"noise_space: {name} has shape {list(t.shape)} for {total} utterances")
    return trajectory[:, start:stop].contiguous(), noise[:, start:stop].contiguous()


def sample_sharded(sample_fn, encoder_hidden_states, cond_masks, total_utterances, chunks=7, group=None, modality_weights=None,
                   source_latents=None, keep_mask=None, tie=None, noise_space=None):
    """Run ``sample_fn(enc_shard, masks_shard, B=<local>, first_utterance=<global id>)`` on this rank's
    utterances and return the gathered latents [total, L, 128] on every rank.  A ``sample_fn`` with ``operands="auto"`` decides PER RANK:
    each rank's census sees its own utterances only, so one rank may fall back to ``operands=0`` while another keeps the default policy
    (each shard's result is still bit for bit one of the two policies' for its utterances); no decision is all-reduced.
    ``modality_weights`` (optional): per-modality guidance weights of the whole batch; ``sample_fn`` then also gets
    ``modality_weights=`` with this rank's utterances (``shard_modality_weights``).  ``source_latents`` [total, L, 128] / ``keep_mask``
    [total, L] (optional, an edit run): ``sample_fn`` gets this rank's rows of each under the same names.  ``tie`` [total, L] (optional,
    a tied run): ``sample_fn`` gets ``tie=`` with this rank's rows renumbered to its slice (``shard_tie``); a tie that crosses the slice is
    refused -- keep the rows that are tied to each other (the windows of one utterance) on one rank.  ``noise_space`` (optional, the
    replay of an edit-friendly DDPM noise space): the pair (trajectory [N + 1, total, L, 128], noise [N, total, L, 128]); ``sample_fn`` gets
    ``noise_space=`` with this rank's rows of both rings (``shard_noise_space``), next to its rows of ``keep_mask``."""
    ws = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    a, b = shard_range(total_utterances, rank, ws)
    enc = [shard_cfg_batch(m, a, b, total_utterances, chunks) for m in encoder_hidden_states]
    masks = {k: shard_cfg_batch(v, a, b, total_utterances, chunks) for k, v in (cond_masks or {}).items()}
    extra = {}
    if modality_weights is not None:
        extra["modality_weights"] = shard_modality_weights(modality_weights, a, b, total_utterances)
    for name, t in (("source_latents", source_latents), ("keep_mask", keep_mask)):
        if t is not None:
            if t.shape[0] != total_utterances:
                raise ValueError(f"{name} has {t.shape[0]} rows for {total_utterances} utterances")
            extra[name] = t[a:b]
    if tie is not None:
        extra["tie"] = shard_tie(tie, a, b, total_utterances)
    if noise_space is not None:
        extra["noise_space"] = shard_noise_space(noise_space, a, b, total_utterances)
    local = sample_fn(enc, masks, B=b - a, first_utterance=a, **extra)
    return gather_latents(local, total_utterances, group)
