"""BERT4RecModel: the Keras-model surface of bert4rec/models/bert4rec_model.py:27-240 on the HIP engine.

  model(inputs, training=)   -> dict(sequence_output, pooled_output, encoder_outputs, mlm_logits)   :110-149
  model.compile / fit / train_step / test_step                                                      :151-192
  model.rank_items(encoder_input, items)                                                            :203-240

The arithmetic runs in libb4r_hip.so (include/b4r.h); this class only sequences calls and keeps the Keras bookkeeping
(metric names and averaging rules, History, callbacks)."""
from __future__ import annotations

import numbers
from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .. import activations
from .. import engine as engine_mod
from ..trainers import trainer_utils
from ..trainers.optimizers import AdamWeightDecay
from ..trainers import optimizers as _optimizers
from .components import networks

SPECIAL_TOKEN_IDS = [0, 1, 2]  # [PAD], [MASK], [UNK]: bert4rec_dataloader.py:38-43


class History:
    """Minimal stand-in for the object Keras fit() returns (bert4rec_trainer.py:62-68)."""

    def __init__(self):
        self.history: Dict[str, List[float]] = {}
        self.epoch: List[int] = []

    def _append(self, epoch: int, logs: Dict[str, float]):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


class _MetricLog:
    """Per-step copies of the 64-byte device state; read back once (no host sync inside the step loop)."""

    def __init__(self, device, capacity: int = 1024):
        self.device = device
        self.buf = torch.zeros((capacity, _lib.STATE_WORDS), dtype=torch.int32, device=device)
        self.n = 0
        self.batch_sizes: List[int] = []

    def reset(self):
        self.n = 0
        self.batch_sizes = []

    def push(self, state: torch.Tensor, batch_size: Optional[int]):
        """batch_size None (data-parallel rounds): the weight of the round in the epoch's loss is the all-reduced slot count of the
        state (rows of the JOINED batch x P) -- the same on every rank, also on one that had no batch in the round"""
        if self.n == self.buf.shape[0]:
            bigger = torch.zeros((2 * self.buf.shape[0], _lib.STATE_WORDS), dtype=torch.int32, device=self.device)
            bigger[: self.n].copy_(self.buf[: self.n])
            self.buf = bigger
        self.buf[self.n].copy_(state, non_blocking=True)
        self.n += 1
        self.batch_sizes.append(-1 if batch_size is None else batch_size)

    def results(self, prefix: str = "") -> Dict[str, float]:
        """Keras averaging rules: `loss` = batch-size-weighted mean of the per-batch losses; SparseCategoricalAccuracy =
        matches / slots over the epoch; masked_accuracy (a plain function metric) = unweighted mean of per-batch values."""
        if self.n == 0:
            return {}
        f = self.buf[: self.n].cpu().view(torch.float32).numpy().astype(np.float64)
        bs = np.asarray(self.batch_sizes, dtype=np.float64)
        bs = np.where(bs < 0, f[:, _lib.ST_SLOTS_ALL], bs)
        loss_b = f[:, _lib.ST_LOSS_SUM] / f[:, _lib.ST_VALID]
        macc_b = f[:, _lib.ST_CORRECT_MASKED] / f[:, _lib.ST_VALID]
        return {prefix + "loss": float((loss_b * bs).sum() / bs.sum()),
                prefix + "sparse_categorical_accuracy": float(f[:, _lib.ST_CORRECT_ALL].sum() / f[:, _lib.ST_SLOTS_ALL].sum()),
                prefix + "masked_accuracy": float(macc_b.mean())}


class BERT4RecModel:
    def __init__(self, encoder: networks.Bert4RecEncoder, customized_masked_lm: Any = None, mlm_activation="gelu",
                 mlm_initializer="glorot_uniform", name: str = "bert4rec",
                 special_token_ids: Optional[List[int]] = SPECIAL_TOKEN_IDS, **kwargs):
        if customized_masked_lm is not None:
            raise NotImplementedError("customized_masked_lm is not supported: the masked-LM head is a fused HIP path")
        mlm_id = activations.activation_id(mlm_activation, "mlm_activation")
        # the transform's activation lives in the encoder's engine: a second model on the same encoder may not switch it
        bound = getattr(encoder.engine, "_mlm_activation_bound", None)   # (id, name) of the first model on this encoder
        if bound is not None and bound[0] != mlm_id:
            raise ValueError(f"mlm_activation={mlm_activation!r}: this encoder already serves a model with mlm_activation={bound[1]!r}")
        encoder.engine.set_mlm_activation(mlm_id)
        encoder.engine._mlm_activation_bound = (mlm_id, mlm_activation)
        self._config = {"encoder": encoder, "customized_masked_lm": customized_masked_lm,
                        "mlm_activation": mlm_activation, "mlm_initializer": mlm_initializer, "name": name}
        self.name = name
        self.encoder = encoder
        self.engine = encoder.engine
        self.device = encoder.device
        self.vocab_size = encoder.get_config()["vocab_size"]
        # the reference builds a -inf prediction mask for the special tokens and then disables it
        # (bert4rec_model.py:89-102): PAD/MASK/UNK logits are NOT suppressed.
        self.prediction_mask = None
        self.special_token_ids = special_token_ids
        self.inputs = ["input_word_ids", "input_mask", "masked_lm_positions"]
        self.optimizer: Optional[AdamWeightDecay] = None
        self.loss = None
        self.compiled_loss = None
        self.compiled_metrics = None
        self.metrics_names = ["loss", "sparse_categorical_accuracy", "masked_accuracy"]
        self.stop_training = False
        self._hp = None
        self._train_log = _MetricLog(self.device) if self.device.type == "cuda" else None
        self._eval_log = _MetricLog(self.device) if self.device.type == "cuda" else None
        self._trained_steps = 0

    @property
    def identifier(self):
        return "bert4rec"

    # ---- forward ------------------------------------------------------------------------------------------------------
    def __call__(self, inputs, training=None, mask=None) -> Dict[str, Any]:
        if isinstance(inputs, (list, tuple)):
            inputs = dict(zip(self.inputs, inputs))
        cb, keep = self.engine.prepare_batch(inputs)
        self.engine.forward(cb, training=bool(training), pooler=True)
        return self._outputs(cb)

    call = __call__

    def _outputs(self, cb, copy: bool = True) -> Dict[str, Any]:
        """bert4rec_model.py:139-149.  copy=True (the public call): tensors of their own, as the reference returns; the engine's
        workspace is overwritten by the next forward / train_step / test_step of the same batch shape."""
        out = self.encoder._outputs(cb, copy)
        if cb.P > 0:
            B, L, P = cb.B, cb.L, cb.P
            # [B,P,V] view into the (row-padded) logits buffer: values as in the reference, strides differ
            logits = self.engine.region("mlm_logits", B, L, P)
            view = torch.as_strided(logits, (B, P, self.vocab_size), (P * logits.stride(0), logits.stride(0), 1),
                                    logits.storage_offset())
            out["mlm_logits"] = view.contiguous() if copy else view
        return out

    # ---- compile / steps ------------------------------------------------------------------------------------------------
    def compile(self, optimizer=None, loss=None, metrics=None):
        """bert4rec_trainer.py:13-35.  Only the reference's own loss/metric set is fused on the device."""
        optimizer = _optimizers.get(optimizer if optimizer is not None else "adamw")
        if loss is None:
            loss = trainer_utils.MaskedSparseCategoricalCrossentropy()
        if not isinstance(loss, trainer_utils.MaskedSparseCategoricalCrossentropy):
            raise NotImplementedError("only MaskedSparseCategoricalCrossentropy is implemented as a fused device loss")
        self.optimizer = optimizer
        self.loss = self.compiled_loss = loss
        self.compiled_metrics = metrics if metrics is not None else ["sparse_categorical_accuracy", trainer_utils.masked_accuracy]
        self._hp = optimizer.kernel_config(self.engine.table, self.engine.n_params, self.engine.device)

    def _require_compiled(self):
        if self._hp is None:
            raise RuntimeError("The model needs to be compiled first (trainers.get(model=model).initialize_model()).")

    def _enqueue_train_step(self, cb, group=None):
        if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                 and torch.distributed.get_world_size() > 1):
            self.engine.dp_train_step(self._hp, cb, group)
        else:
            self.engine.train_step(self._hp, cb)
        self._trained_steps += 1
        self.optimizer.iterations += 1

    def train_step(self, inputs) -> Dict[str, float]:
        """bert4rec_model.py:151-173.  Returns the running epoch metrics like Keras does."""
        self._require_compiled()
        cb, keep = self.engine.prepare_batch(inputs)
        if cb.P == 0 or keep.get("masked_lm_ids") is None:
            raise ValueError("train_step needs masked_lm_positions and masked_lm_ids")
        self._enqueue_train_step(cb)
        self._train_log.push(self.engine.state, cb.B)
        return self._train_log.results()

    def _enqueue_test_step(self, cb):
        # loss + the two accuracies only: the logits-free head where it exists (no [B*P, V] tensor is written)
        fused = self.engine.fused_head_supported()
        self.engine.begin_step()
        self.engine.forward(cb, training=False, pooler=False, fused_head=fused)
        self.engine.loss(cb, want_grad=False, fused_head=fused)

    def test_step(self, inputs) -> Dict[str, float]:
        """bert4rec_model.py:175-192"""
        cb, keep = self.engine.prepare_batch(inputs)
        if cb.P == 0 or keep.get("masked_lm_ids") is None:
            raise ValueError("test_step needs masked_lm_positions and masked_lm_ids")
        self._enqueue_test_step(cb)
        self._eval_log.push(self.engine.state, cb.B)
        return self._eval_log.results()

    def reset_metrics(self):
        self._train_log.reset()
        self._eval_log.reset()

    def evaluate(self, x: Iterable, steps: Optional[int] = None, prefix: str = "") -> Dict[str, float]:
        self._eval_log.reset()
        for i, batch in enumerate(x):
            if steps is not None and i >= steps:
                break
            cb, keep = self.engine.prepare_batch(batch)
            self._enqueue_test_step(cb)
            self._eval_log.push(self.engine.state, cb.B)
        return self._eval_log.results(prefix)

    def fit(self, x: Iterable, validation_data: Optional[Iterable] = None, epochs: int = 1, callbacks: Sequence = (),
            steps_per_epoch: Optional[int] = None, validation_steps: Optional[int] = None, verbose: int = 1) -> History:
        """Keras fit() as the reference drives it (bert4rec_trainer.py:62-68): per epoch all batches of `x`, then the
        validation pass; callbacks see the Keras metric names (val_masked_accuracy, ...)."""
        self._require_compiled()
        for ds in (x, validation_data):
            if ds is not None and hasattr(ds, "cache_on_device"):
                ds.cache_on_device(self.device)
        history = History()
        self.stop_training = False
        for cb_ in callbacks:
            if hasattr(cb_, "set_model"):
                cb_.set_model(self)
        rank, world = _dp_rank_world()
        if world > 1:   # data parallel: the ranks take the batches of an epoch in turn (same number each), with their own dropout masks
            if not hasattr(x, "__len__"):
                raise ValueError("data-parallel fit() needs a sized training set (every rank must take the same number of steps)")
            if not getattr(self, "_dp_seeded", False):
                self.engine.set_seed(self.engine.read_state()["seed"] + rank)
                self._dp_seeded = True
        for epoch in range(epochs):
            self._train_log.reset()
            for i, batch in enumerate(dp_shard(x, rank, world)):
                if steps_per_epoch is not None and i >= steps_per_epoch:
                    break
                if batch is None:      # the last round of the epoch has no batch for this rank: zero contribution, same update
                    self.engine.dp_idle_step(self._hp)
                    self._trained_steps += 1
                    self.optimizer.iterations += 1
                    self._train_log.push(self.engine.state, None)
                    continue
                cb, keep = self.engine.prepare_batch(batch)
                self._enqueue_train_step(cb)
                self._train_log.push(self.engine.state, cb.B if world == 1 else None)
            logs = self._train_log.results()
            if validation_data is not None:
                logs.update(self.evaluate(validation_data, validation_steps, prefix="val_"))
            history._append(epoch, logs)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs} - " + " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()), flush=True)
            for cb_ in callbacks:
                if hasattr(cb_, "on_epoch_end"):
                    cb_.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        for cb_ in callbacks:
            if hasattr(cb_, "on_train_end"):
                cb_.on_train_end()
        return history

    # ---- ranking ----------------------------------------------------------------------------------------------------------
    def _ranked_slot_hidden(self, encoder_input: Dict[str, torch.Tensor], slots: Optional[torch.Tensor] = None,
                            rows: Optional[torch.Tensor] = None):
        """Encoder forward (no logits, no head on the slots nobody ranks), then tfm MaskedLM's transform on the R slots with
        masked_lm_weights == 1 only (all slots when the key is absent).  The reference computes all [B, P, V] logits and
        keeps the valid slots afterwards (bert4rec_model.py:215-220).  Returns (hidden [R,H], slot index [R] = b*P+p,
        valid slots per batch row).  slots: the caller already has the slot indices (the evaluator, from sampling the candidates):
        nothing is read back to the host here, and the per-row counts are not formed (None)."""
        cb, keep = self.engine.prepare_batch(encoder_input)
        if cb.P == 0:
            raise ValueError("rank_items needs masked_lm_positions")
        B, L, P = cb.B, cb.L, cb.P
        # rows given: the caller vouches that the ranked slots are exactly the slots with masked_lm_ids != 0 (the evaluator checks it
        # once per resident batch) -- the last layer's feed-forward half then runs on those rows only
        enc = self.engine.encoder_forward(cb, training=False, ranked_rows_only=rows is not None and "masked_lm_ids" in keep)
        counts = None
        if slots is None:
            if "masked_lm_weights" in encoder_input and encoder_input["masked_lm_weights"] is not None:
                w = torch.as_tensor(encoder_input["masked_lm_weights"]).to(self.device).reshape(B, P) != 0
            else:
                w = torch.ones((B, P), dtype=torch.bool, device=self.device)
            slots = torch.nonzero(w.reshape(-1), as_tuple=False).reshape(-1)  # row-major => batch order, then slot order
            counts = w.sum(dim=1).tolist()
        if slots.numel() == 0:
            return None, slots, counts
        if rows is None:                                                           # (the evaluator keeps them for resident batches)
            pos = keep["masked_lm_positions"].reshape(-1)[slots].clamp(0, L - 1)   # tfm MaskedLM gathers position + b*L
            rows = torch.div(slots, P, rounding_mode="floor") * L + pos
        seq = self.engine.region("sequence_output", B, L, enc.P, encoder_only=enc.P > 0)   # (P > 0: the ranked-rows forward's own buffer)
        return self.engine.mlm_transform_rows(seq, rows), slots, counts

    def rank_items_tensor(self, encoder_input: Dict[str, torch.Tensor], candidates: Optional[torch.Tensor] = None,
                          ground_truth: Optional[torch.Tensor] = None, want_ranking: bool = True,
                          slots: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        """Device-side core of rank_items: b4r_rank_candidates on every slot with masked_lm_weights == 1.  candidates:
        [R, C] int64 or None (whole vocabulary, ranked without materialising an [R, V] candidate list).
        Returns (ranking [R,C] int64, gt_rank [R] int32 or None, slot_index [R] int64 (b*P+p), rows_per_batch_entry (None when the
        caller passed `slots`))."""
        hidden, slots, counts = self._ranked_slot_hidden(encoder_input, slots, rows)
        R = int(slots.numel())
        if R == 0:
            return None, None, slots, counts
        if candidates is not None:
            candidates = torch.as_tensor(candidates).to(device=self.device, dtype=torch.int64).contiguous()
            if candidates.shape[0] != R:
                raise ValueError(f"{candidates.shape[0]} candidate lists for {R} masked slots")
        ranking, gt_rank, _ = self.engine.rank_candidates(hidden, None, candidates, ground_truth, want_ranking=want_ranking,
                                                          n_candidates=self.vocab_size, n_rows=R)
        return ranking, gt_rank, slots, counts

    def rank_items(self, encoder_input: dict, items: list = None):
        """bert4rec_model.py:203-240.  `items`: per batch row a list (one entry per masked slot) of candidate-id lists;
        returns per batch row a list of 1-D tensors: the candidates sorted by descending logit (ties: lower index first)."""
        cand = None
        if items is not None and len(items) > 0 and type(items[0]) is list:
            flat = [c for row in items for c in row]
            lens = {len(c) for c in flat}
            if len(lens) > 1:
                return self._rank_items_ragged(encoder_input, items)
            cand = torch.tensor(flat, dtype=torch.int64)
        ranking, _, slots, counts = self.rank_items_tensor(encoder_input, cand)
        out, r = [], 0
        for n in counts:
            out.append([ranking[r + j] for j in range(n)])
            r += n
        return out

    def recommend_tensor(self, encoder_input: Dict[str, torch.Tensor], k: int = 10, exclude_seen: bool = True,
                         exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None, diversity: Optional[float] = None,
                         pool: Optional[int] = None, max_per_group=None, return_distribution: bool = False,
                         temperature: float = 1.0, sample_seed: Optional[int] = None, sample_streams=None, calibrate=None,
                         calibration: Optional[float] = None, calibration_alpha: float = 0.01, return_calibration: bool = False):
        """Top k of the whole catalogue for every slot with masked_lm_weights == 1 (all slots when the key is absent), from one
        b4r_rank_full call: no [R, V] scores.  The forward is rank_items_tensor's (encoder, then tfm MaskedLM's transform on those
        slots only).  [PAD] / [MASK] / [UNK] are never recommended; exclude_seen drops the row's own input_word_ids; exclude
        [B, E] int64 (-1 padded): more ids per batch row not to recommend.  Returns (ids [R,k] int64, scores [R,k] fp32,
        slot_index [R] int64 = b*P+p), on the device; a row with fewer than k allowed items ends in -1 / -inf.
        allow: restrict the catalogue -- a bool / uint8 mask [V] (nonzero = may be recommended), masks [F, V] with row_filter [R]
        (the filter of each ranked row; an index outside [0, F) = no filter), or packed uint32 [F, ceil(V / 32)]
        (bert4rec_amd.apps.pack_item_filter).  The filter is applied inside the sweep (b4r_rank_full_ex).
        diversity: None = the plain top k.  A number d in [0, 1]: the sweep returns the best `pool` allowed items of every row
        (default min(1024, max(10 k, 50)); at least k) and b4r_rerank_diverse picks k of them by greedy Maximal Marginal Relevance
        with lambda = 1 - d and cosine similarity in the item table: 0 keeps the plain order, 1 ranks by dissimilarity to the items
        already picked alone.  The scores returned are the picked items' sweep scores (no longer descending).
        max_per_group: None, one bert4rec_amd.apps.pack_item_groups spec or a list of at most 4 -- "at most c items per category /
        brand / ...".  The sweep returns the best `pool` allowed items of every row (the same default) and b4r_rerank_quota picks k of
        them greedily under the caps: in relevance order when diversity is None (lambda = 1), else by MMR as above.  A row whose pool
        holds fewer than k admissible items ends in -1 / -inf: there is no second, wider sweep (it would need a host
        synchronisation); a larger `pool` is the remedy.
        return_distribution: a fourth value follows, score_distribution_tensor's dict for the same rows, exclusions and filter at
        `temperature` (b4r_score_dist, one more sweep): its logp [R, k] holds the log probabilities of the ids returned,
        after the re-ranking when one is on (-inf under the -1 tail).  ids and scores are the call's without it, bit for bit.
        A temperature other than 1.0 without return_distribution or sample_seed raises ValueError.
        sample_seed: None = the deterministic top k.  An integer in [0, 2^64): the k items are DRAWN without replacement from
        softmax(scores / temperature) over the slot's allowed catalogue (b4r_sample_full: one sweep with Gumbel-perturbed keys, no
        [R, V] scores); with pool = M the draw is over the best M allowed items instead (b4r_rank_full, then b4r_sample_pool).  The
        ids come in draw order and the scores keep b4r_rank_full's bits (not descending).  sample_streams [R] int64: the noise
        stream of each ranked slot (None: the slot's row number 0 .. R-1); the same (sample_seed, stream) draws the same list
        whatever else the batch holds.  With return_distribution the log probabilities are b4r_score_dist's at the same temperature:
        they are over the slot's FULL allowed catalogue, also when `pool` truncates the draw.  sample_seed together with diversity
        or max_per_group raises ValueError.
        calibrate: None, or (item_groups, n_groups, target) -- the k items are picked from the best `pool` allowed items of every row
        (the same default) so that the list's shares of the item groups follow the row's target distribution (b4r_rerank_calibrated:
        Steck's calibrated recommendations; "70 % drama and 30 % comedy in, 70 / 30 out").  item_groups / n_groups: one label per
        token id as group_affinity_tensor takes them, at most 1024 groups.  target: "history" = per ranked slot the count of each
        label among the row's input_word_ids (special ids and unlabelled items are not counted; formed on the device without a
        synchronisation); "affinity" = group_affinity_tensor's group_mass of the same forward, exclusions and filter (two more
        sweeps); or an int64 tensor [R, G] of non-negative masses in any unit.  calibration: lambda in [0, 1] (default 0.5): 0
        returns the plain top k, 1 picks by the calibration gain alone.  calibration_alpha in (0, 1): the smoothing of the list's
        shares towards the target.  return_calibration: one more value follows (after the distribution's dict when both are asked
        for): {"kl": float64 [R], the miscalibration KL(target || smoothed shares of the list) of every returned list, NaN for a row
        without a target or without an item; "target_mass": int64 [R, G], the target used}.  calibrate together with diversity,
        max_per_group or sample_seed raises ValueError, and so do calibration or return_calibration without calibrate."""
        k = engine_mod.check_rank_full_args(k, exclude)
        cal = None
        if calibrate is not None:
            if diversity is not None or max_per_group is not None or sample_seed is not None:
                raise ValueError("calibrate does not combine with diversity, max_per_group or sample_seed")
            cal = engine_mod.check_calibrate(calibrate, self.vocab_size)
        elif calibration is not None or return_calibration:
            raise ValueError("calibration and return_calibration belong to the calibrated re-ranking: give calibrate as well")
        sampled = sample_seed is not None
        if sampled:
            sample_seed = engine_mod.check_sample_seed(sample_seed)
            if diversity is not None or max_per_group is not None:
                raise ValueError("sample_seed does not combine with diversity or max_per_group")
            sample_streams = engine_mod.check_sample_streams(sample_streams)
            if pool is not None:
                k, pool = engine_mod.check_sample_pool_args(k, pool)
        elif sample_streams is not None:
            raise ValueError("sample_streams are the noise streams of a sampled call: give sample_seed as well")
        if not return_distribution and not sampled and not (isinstance(temperature, numbers.Real) and temperature == 1.0):
            raise ValueError("temperature scales the returned distribution: give return_distribution=True or sample_seed as well")
        engine_mod.check_temperature(temperature)
        n_sweep = k
        quotas = engine_mod.check_quota_args(max_per_group, self.vocab_size) if max_per_group is not None else None
        if quotas is not None:
            k, n_sweep, _ = engine_mod.check_rerank_args(k, pool, 0.0 if diversity is None else diversity)
        elif diversity is not None:
            k, n_sweep, _ = engine_mod.check_rerank_args(k, pool, diversity)
        elif cal is not None:
            k, n_sweep, cal_lambda, cal_alpha = engine_mod.check_calibration_args(k, pool, 0.5 if calibration is None else calibration,
                                                                                  calibration_alpha)
        elif pool is not None and not sampled:
            raise ValueError("pool is the candidate count of the re-ranking: give diversity, max_per_group, calibrate or sample_seed as well")
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        dev = self.device
        if hidden is None:
            out = (torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev), slots)
            if return_distribution:
                out += (self._distribution_dict(None, slots, k),)
            if return_calibration:
                out += ({"kl": torch.empty((0,), dtype=torch.float64, device=dev),
                         "target_mass": torch.empty((0, cal[1]), dtype=torch.int64, device=dev)},)
            return out
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        if sampled and pool is None:
            ids, scores, _ = self.engine.sample_full(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, k, sample_seed, allow, row_filter,
                                                     temperature, sample_streams)
        else:
            ids, scores, _ = self.engine.rank_full(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, pool if sampled else n_sweep,
                                                   allow, row_filter)
        if sampled and pool is not None:
            ids, scores, _, _ = self.engine.sample_pool(ids, scores, k, sample_seed, temperature, sample_streams)
        elif quotas is not None:
            ids, scores, _, _ = self.engine.rerank_quota(ids, scores, k, 0.0 if diversity is None else diversity, quotas)
        elif diversity is not None:
            ids, scores, _ = self.engine.rerank_diverse(ids, scores, k, diversity)
        elif cal is not None:
            labels_d = cal[0].to(dev)
            target = self._calibration_target(cal[2], encoder_input, slots, hidden, ex_rows, labels_d, cal[1], allow, row_filter, temperature)
            ids, scores, _, _, kl = self.engine.rerank_calibrated(ids, scores, k, cal_lambda, labels_d, cal[1], target, cal_alpha)
        out = (ids, scores, slots)
        if return_distribution:
            dist = self.engine.score_distribution(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, allow, row_filter, temperature, ids)
            out += (self._distribution_dict(dist, slots, k),)
        if return_calibration:
            out += ({"kl": kl, "target_mass": target},)
        return out

    def _calibration_target(self, target, encoder_input, slots: torch.Tensor, hidden, ex_rows, labels_d: torch.Tensor, G: int, allow,
                            row_filter, temperature) -> torch.Tensor:
        """The target masses int64 [R, G] of a calibrated re-ranking on the device: the label counts of every ranked slot's own
        input_word_ids ("history"), _group_affinity's masses of the same rows ("affinity"), or the caller's tensor."""
        R = int(slots.numel())
        if isinstance(target, str) and target == "history":
            P = int(torch.as_tensor(encoder_input["masked_lm_positions"]).shape[1])
            tokens = torch.as_tensor(encoder_input["input_word_ids"]).to(device=self.device, dtype=torch.int64)
            return engine_mod.group_history_counts(tokens[torch.div(slots, P, rounding_mode="floor")], labels_d, G)
        if isinstance(target, str):
            return self._group_affinity(hidden, ex_rows, labels_d, G, allow, row_filter, temperature)["group_mass"]
        if int(target.shape[0]) != R:
            raise ValueError(f"the calibration target holds {int(target.shape[0])} rows for {R} ranked slots")
        return target.to(self.device).contiguous()

    def _excluded_rows(self, encoder_input, slots: torch.Tensor, exclude_seen: bool, exclude) -> Optional[torch.Tensor]:
        """The exclude list of every ranked slot [R, E]: the row's own input_word_ids (exclude_seen) and / or its row of `exclude`."""
        dev = self.device
        P = int(torch.as_tensor(encoder_input["masked_lm_positions"]).shape[1])
        b_idx = torch.div(slots, P, rounding_mode="floor")
        parts = []
        if exclude_seen:
            parts.append(torch.as_tensor(encoder_input["input_word_ids"]).to(device=dev, dtype=torch.int64)[b_idx])
        if exclude is not None:
            ex = torch.as_tensor(exclude).to(device=dev, dtype=torch.int64)
            B = int(torch.as_tensor(encoder_input["input_word_ids"]).shape[0])
            if ex.shape[0] != B:
                raise ValueError(f"exclude has {ex.shape[0]} rows for a batch of {B}")
            parts.append(ex[b_idx])
        return torch.cat(parts, dim=1) if parts else None

    def _distribution_dict(self, dist, slots: torch.Tensor, K: Optional[int]) -> Dict[str, torch.Tensor]:
        """Engine.score_distribution's tuple (None: no ranked slot) as score_distribution_tensor's dict"""
        dev = self.device
        if dist is None:
            n = torch.empty((0,), dtype=torch.int32, device=dev)
            lse = ent = torch.empty((0,), dtype=torch.float64, device=dev)
            logp = None if K is None else torch.empty((0, K), dtype=torch.float32, device=dev)
        else:
            n, _, lse, ent, logp = dist
        return {"n": n, "lse": lse, "entropy": ent, "perplexity": torch.exp(ent), "logp": logp, "slot_index": slots}

    def score_distribution_tensor(self, encoder_input: Dict[str, torch.Tensor], query_ids=None, exclude_seen: bool = True,
                                  exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None, temperature: float = 1.0):
        """The softmax over the catalogue each ranked slot could have been served -- recommend_tensor's forward, exclusions
        (exclude_seen, exclude; [PAD] / [MASK] / [UNK] never count) and filter (allow, row_filter) -- from one b4r_score_dist call: no
        [R, V] scores.  The scores are divided by `temperature` (finite, > 0).  query_ids [R, K] int64 (K <= 1024) or None: the items
        whose log probability is wanted, one list per ranked slot.  Returns a dict of device tensors, one entry per ranked slot:
          n           int32: the items the slot could have been served
          lse         float64: the log normaliser of the scaled scores
          entropy     float64: the entropy of the distribution in nats (0 where n = 0)
          perplexity  float64: exp(entropy), between 1 (one item holds all the mass) and n (uniform)
          logp        float32 [R, K]: the log probability of each queried id, -inf where the slot could not be served it (None
                      without query_ids)
          slot_index  int64: b*P+p, as recommend_tensor returns it."""
        engine_mod.check_temperature(temperature)
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        if hidden is None:
            return self._distribution_dict(None, slots, None if query_ids is None else int(torch.as_tensor(query_ids).shape[-1]))
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        dist = self.engine.score_distribution(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, allow, row_filter, temperature,
                                              query_ids)
        return self._distribution_dict(dist, slots, None)

    def item_ranks_tensor(self, encoder_input: Dict[str, torch.Tensor], query_ids, exclude_seen: bool = True,
                          exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None, members: str = "strict"):
        """Where given items stand for every ranked slot -- recommend_tensor's forward, exclusions (exclude_seen, exclude; [PAD] /
        [MASK] / [UNK] never count) and filter (allow, row_filter) -- from one forward and one b4r_item_ranks call: no [R, V] scores
        and no sweep per item.  query_ids: int64 [R, Q], one list per ranked slot (any id outside the vocabulary, such as -1, is
        padding), or [Q] for all slots.  members: "strict" (an item the slot could not be served has no rank), "self" (every item is
        ranked against the servable ones, as the full-ranking evaluation ranks its target) or "joint" (the slot's items are ranked
        in one list together with the servable ones; at most 256 columns).  More than 256 columns are served in blocks of 256 under
        "strict" / "self", whose columns do not depend on each other.  Returns a dict of device tensors, one entry per ranked slot:
          ranks       int32 [R, Q]: the 1-based position of the item in recommend_tensor's order (ties to the lower id); 0 = none
          scores      float32 [R, Q]: the item's score, -inf for an id outside the vocabulary
          n           int32 [R]: the size of the ranked set ("of n")
          member      uint8 [R, Q]: 1 where the slot could be served the item
          slot_index  int64 [R]: b*P+p, as recommend_tensor returns it."""
        q = torch.as_tensor(query_ids)
        flat = q.ndim == 1
        q, Q, _ = engine_mod.check_item_ranks_args(q.reshape(1, -1) if flat else q, None, members, None)
        if members == "joint" and Q > engine_mod.ITEM_RANKS_MAX_Q:
            raise ValueError(f'members="joint" ranks at most {engine_mod.ITEM_RANKS_MAX_Q} items per slot in one list, got {Q}')
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        R = int(slots.numel())
        if flat:
            q = q.expand(R, Q)
        elif q.shape[0] != R:
            raise ValueError(f"query_ids has {q.shape[0]} rows for {R} ranked slots")
        dev = self.device
        if hidden is None:
            return {"ranks": torch.empty((0, Q), dtype=torch.int32, device=dev), "scores": torch.empty((0, Q), dtype=torch.float32, device=dev),
                    "n": torch.empty((0,), dtype=torch.int32, device=dev), "member": torch.empty((0, Q), dtype=torch.uint8, device=dev),
                    "slot_index": slots}
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        q = q.to(dev)
        block = engine_mod.ITEM_RANKS_MAX_Q
        parts = [self.engine.item_ranks(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, q[:, c:c + block].contiguous(), members, allow, row_filter)
                 for c in range(0, max(Q, 1), block)]
        if len(parts) == 1:
            ranks, scores, n, member = parts[0]
        else:
            ranks, scores, member = (torch.cat([p[i] for p in parts], dim=1) for i in (0, 1, 3))
            n = parts[0][2]
        return {"ranks": ranks, "scores": scores, "n": n, "member": member, "slot_index": slots}

    def item_ranks(self, encoder_input: dict, items):
        """item_ranks_tensor for one sequence with one ranked slot, as Python values: a list with one {"item", "rank", "of", "score"}
        per id of `items` (rank None for an id the slot cannot be served or the vocabulary does not hold)."""
        got = self.item_ranks_tensor(encoder_input, torch.as_tensor(list(items), dtype=torch.int64).reshape(-1))
        if got["ranks"].shape[0] != 1:
            raise ValueError(f"item_ranks serves one ranked slot, the input has {got['ranks'].shape[0]}; use item_ranks_tensor")
        ranks, scores, n = got["ranks"][0].cpu().tolist(), got["scores"][0].cpu().tolist(), int(got["n"][0])
        return [{"item": int(i), "rank": r if r > 0 else None, "of": n, "score": s} for i, r, s in zip(items, ranks, scores)]

    def list_metrics_tensor(self, ids: torch.Tensor, ground_truth: Optional[torch.Tensor] = None,
                            item_weight: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Beyond-accuracy metrics of recommendation lists ids [R, K] int64 (recommend_tensor's ids, re-ranked or not; -1 entries are
        skipped), from one b4r_list_metrics call in the item table.  Returns device tensors, one entry per list:
          n        int32: the items of the list
          ild      float64: intra-list diversity, the mean of 1 - cosine over the list's item pairs; NaN where n < 2
          novelty  float64: the mean item_weight of the list's items (item_weight [V] fp32: the items' self-information,
                   bert4rec_amd.apps.item_self_information); NaN where n < 1 or item_weight is None
          hit_pos  int32: the 1-based position of ground_truth [R] in the list, 0 where absent or ground_truth is None."""
        ids = torch.as_tensor(ids)
        gt = None if ground_truth is None else torch.as_tensor(ground_truth).to(torch.int64)
        w = None if item_weight is None else torch.as_tensor(item_weight)
        n, dist, nov, hit = self.engine.list_metrics(ids, gt, w)
        n64 = n.to(torch.float64)
        nan = torch.full_like(n64, float("nan"))
        pairs = n64 * (n64 - 1.0) / 2.0
        ild = torch.where(n >= 2, (dist.to(torch.float64) / 2.0 ** 30) / pairs.clamp(min=1.0), nan)
        novelty = nan if w is None else torch.where(n >= 1, (nov.to(torch.float64) / 2.0 ** 30) / n64.clamp(min=1.0), nan)
        return {"n": n, "ild": ild, "novelty": novelty, "hit_pos": hit}

    def similar_items_tensor(self, item_ids, k: int = 10, metric: str = "cosine", allow=None, row_filter=None):
        """Item-to-item neighbours in the encoder's item table (the tied output embedding, width E when factorised): for each of
        item_ids [R] the k nearest items by metric "cosine" or "dot", the item itself and [PAD] / [MASK] / [UNK] left out, ties to
        the lower id; allow / row_filter as in recommend_tensor.  Returns (ids [R,k] int64, scores [R,k] fp32) on the device; an
        id that is no item gives a row of -1 / -inf.  One b4r_item_neighbours call: no [R, V] scores."""
        return self.engine.item_neighbours(item_ids, k, metric, engine_mod.SPECIAL_IDS, allow, row_filter)

    def recommend(self, encoder_input: dict, k: int = 10, exclude_seen: bool = True, exclude=None, diversity: Optional[float] = None,
                  pool: Optional[int] = None, max_per_group=None, return_distribution: bool = False,
                  temperature: float = 1.0, sample_seed: Optional[int] = None, sample_streams=None, calibrate=None,
                  calibration: Optional[float] = None, calibration_alpha: float = 0.01, return_calibration: bool = False):
        """recommend_tensor as Python lists: per batch row, one list per ranked slot of (ids, scores) lists of length k.
        return_distribution: the entries are (ids, scores, log probabilities) instead, and recommend_tensor's dict follows as a second
        return value (device tensors).  calibrate / calibration / calibration_alpha: recommend_tensor's; return_calibration: its
        dict of device tensors follows as the last return value."""
        got = self.recommend_tensor(encoder_input, k, exclude_seen, exclude, diversity=diversity, pool=pool,
                                    max_per_group=max_per_group, return_distribution=return_distribution, temperature=temperature,
                                    sample_seed=sample_seed, sample_streams=sample_streams, calibrate=calibrate, calibration=calibration,
                                    calibration_alpha=calibration_alpha, return_calibration=return_calibration)
        ids, scores, slots = got[:3]
        B, P = (int(x) for x in torch.as_tensor(encoder_input["masked_lm_positions"]).shape)
        out = [[] for _ in range(B)]
        if not return_distribution:
            for s, i_row, s_row in zip(slots.cpu().tolist(), ids.cpu().tolist(), scores.cpu().tolist()):
                out[s // P].append((i_row, s_row))
            return (out, got[3]) if return_calibration else out
        for s, i_row, s_row, p_row in zip(slots.cpu().tolist(), ids.cpu().tolist(), scores.cpu().tolist(), got[3]["logp"].cpu().tolist()):
            out[s // P].append((i_row, s_row, p_row))
        return (out,) + tuple(got[3:]) if return_calibration else (out, got[3])

    def _one_slot_batch(self, caller: str, encoder_input, exclude, allow, row_filter, max_len: bool = False):
        """What recommend_sequence_tensor and explain_tensor do before their first forward: the checks of exclude [B, E], allow and
        row_filter [B] (before any work), the batch on the device, and check_rollout_batch (the call's one host synchronisation).
        Returns (packed allow or None, row_filter int32 on the device or None, (tokens, mask, positions) on the device, len [B],
        slot_index [B] = b*P+p, the largest row length or None without max_len)."""
        if exclude is not None and torch.as_tensor(exclude).ndim != 2:
            raise ValueError(f"exclude must be rank 2 [rows, ids], got shape {tuple(torch.as_tensor(exclude).shape)}")
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        rows = encoder_input.get("input_word_ids")
        if row_filter is not None and rows is not None and row_filter.numel() != len(rows):
            raise ValueError(f"row_filter has {row_filter.numel()} entries for a batch of {len(rows)}")
        cb, keep = self.engine.prepare_batch(encoder_input)
        if cb.P == 0:
            raise ValueError(f"{caller} needs masked_lm_positions")
        mask, pos = keep["input_mask"], keep["masked_lm_positions"]
        length, slot_p, *longest = engine_mod.check_rollout_batch(mask, pos, encoder_input.get("masked_lm_weights"), return_max_len=max_len)
        slots = torch.arange(cb.B, dtype=torch.int64, device=self.device) * cb.P + slot_p
        rf = None if row_filter is None else row_filter.to(self.device)
        return allow, rf, (keep["input_word_ids"], mask, pos), length, slots, (longest[0] if max_len else None)

    def recommend_sequence_tensor(self, encoder_input: Dict[str, torch.Tensor], steps: int, beams: int = 1, expand: Optional[int] = None,
                                  exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None,
                                  temperature: float = 1.0, sample_seed: Optional[int] = None, sample_streams=None,
                                  return_logp: bool = True):
        """The next `steps` items of every batch row IN ORDER, each one conditioned on the ones before: after every step the chosen
        item is appended to the row on the device (b4r_rollout_advance: the window advances as prepare_inference(history + [item])
        does) and the forward runs again.  Nothing is read back between the steps.
        encoder_input is prepare_inference's format: every batch row has exactly one weighted slot and it gathers the last real
        token (the [MASK] placeholder); anything else raises ValueError.  That check is the call's one host synchronisation.
        Every step's forward is recommend_tensor's, so its scores are the bits recommend_tensor returns for the same rows.  A row's
        exclusions are its input_word_ids (exclude_seen), its row of `exclude` [B, E] and everything picked so far on its own path
        (an item that slid out of the window stays excluded); allow / row_filter [B] apply at every step.
          beams = 1, no sample_seed: greedy -- the step's item is b4r_rank_full's top 1.
          beams = B > 1: beam search -- every beam proposes its `expand` best items (default B; B * expand <= 4096) with their log
            probabilities at `temperature` (b4r_score_dist) and b4r_beam_select keeps the B paths with the largest summed log
            probability, ties to the better parent, then to the better candidate.  Step 0 runs on the batch rows themselves with
            max(expand, B) candidates.  Beams come out best first; all paths have `steps` items, so a beam that cannot be
            extended is dropped whole.
          sample_seed (beams = 1): step t draws one item from softmax(scores / temperature) with b4r_sample_full under the seed
            (sample_seed + t) mod 2^64 and the row's stream (sample_streams [B] int64; None: the row number), so a user rolls out
            the same path whatever batch they ride in, and several roll-outs of one user are that user repeated with other streams.
        Returns (ids [B, beams, steps] int64, step_logp [B, beams, steps] fp32 or None, logp [B, beams] fp32 or None, slot_index [B]
        int64), on the device.  Greedy and sampled paths end in -1 once nothing is left to recommend; a dropped beam is -1 in every
        column.  step_logp holds the log probability of every item among those the row could be served at its step (-inf under a
        -1; None with return_logp=False), logp their fp32 sum in step order, which for beams is the total the search ranked by (None
        for a greedy or sampled call with return_logp=False, which runs no b4r_score_dist)."""
        steps, beams, expand = engine_mod.check_rollout_args(steps, beams, expand, temperature, sample_seed, return_logp)
        sampled = sample_seed is not None
        if sampled:
            sample_seed = engine_mod.check_sample_seed(sample_seed)
        elif sample_streams is not None:
            raise ValueError("sample_streams are the noise streams of a sampled call: give sample_seed as well")
        allow, rf, (tokens, mask, pos), length, slots0, _ = self._one_slot_batch("recommend_sequence_tensor", encoder_input, exclude, allow,
                                                                                  row_filter)
        eng, dev = self.engine, self.device
        (U, L), P = tokens.shape, pos.shape[1]
        if L < 2:
            raise ValueError("a roll-out needs sequences of at least 2 tokens (an item and the placeholder)")
        streams = engine_mod.check_sample_streams(sample_streams, U) if sampled else None
        ids_out = torch.full((U, beams, steps), -1, dtype=torch.int64, device=dev)
        if U == 0:
            lp = torch.empty((U, beams, steps), dtype=torch.float32, device=dev)
            return ids_out, (lp if return_logp else None), (lp[:, :, 0] if return_logp or beams > 1 else None), slots0
        ex0 = self._excluded_rows(encoder_input, slots0, exclude_seen, exclude)
        E0 = 0 if ex0 is None else int(ex0.shape[1])
        tail = torch.full((U, steps), -1, dtype=torch.int64, device=dev)   # column E0 + t takes step t's item
        cur = {"tokens": tokens, "len": length.to(torch.int32), "exclude": tail if ex0 is None else torch.cat([ex0, tail], dim=1).contiguous(),
               "path": None, "path_logp": None}
        batch = {"input_word_ids": tokens, "input_mask": mask, "masked_lm_positions": pos}
        slots = slots0
        first = engine_mod.SPECIAL_IDS
        N = U * beams
        pair = [None, None]
        st = None if streams is None else streams.to(dev)
        want_dist = return_logp or beams > 1
        lp_out = torch.full((U, 1, steps), float("-inf"), dtype=torch.float32, device=dev) if want_dist and beams == 1 else None
        beam_logp = torch.zeros((U, 1), dtype=torch.float32, device=dev)
        for t in range(steps):
            hidden, _, _ = self._ranked_slot_hidden(batch, slots=slots)
            ex = cur["exclude"]
            dst = None
            if beams > 1 or t + 1 < steps:
                dst = pair[t % 2] = pair[t % 2] or eng.rollout_state(N, L, P, E0 + steps, steps, paths=beams > 1)
            if beams > 1:
                cand, _, _ = eng.rank_full(hidden, None, ex, first, None, max(expand, beams) if t == 0 else expand, allow, rf)
                cand_logp = eng.score_distribution(hidden, None, ex, first, None, allow, rf, temperature, cand)[4]
                parent, item, beam_logp, step_logp = eng.beam_select(beam_logp, cand, cand_logp, beams)
                eng.rollout_advance(cur, dst, parent.reshape(-1), item.reshape(-1), step_logp.reshape(-1), 1 if t == 0 else beams, beams,
                                    t, E0 + t)
                if t == 0 and rf is not None:
                    rf = rf.repeat_interleave(beams)   # a beam row inherits its user's filter
            else:
                if sampled:
                    item, _, _ = eng.sample_full(hidden, None, ex, first, None, 1, (sample_seed + t) % (1 << 64), allow, rf, temperature, st)
                else:
                    item, _, _ = eng.rank_full(hidden, None, ex, first, None, 1, allow, rf)
                ids_out[:, 0, t].copy_(item[:, 0])
                if want_dist:
                    lp_out[:, 0, t].copy_(eng.score_distribution(hidden, None, ex, first, None, allow, rf, temperature, item)[4][:, 0])
                if dst is not None:
                    eng.rollout_advance(cur, dst, None, item[:, 0], None, 1, 1, t, E0 + t)
            if dst is not None:
                cur = dst
                batch = {"input_word_ids": dst["tokens"], "input_mask": dst["mask"], "masked_lm_positions": dst["positions"]}
                if t == 0:
                    slots = torch.arange(N, dtype=torch.int64, device=dev) * P
        if beams > 1:
            step_all = cur["path_logp"].view(U, beams, steps)
            return cur["path"].view(U, beams, steps), (step_all if return_logp else None), beam_logp, slots0
        if not want_dist:
            return ids_out, None, None, slots0
        logp = lp_out[:, :, 0].clone()
        for t in range(1, steps):
            logp = logp + lp_out[:, :, t]     # the fp32 sum in step order, as b4r_beam_select forms a beam's total
        return ids_out, lp_out, logp, slots0

    def recommend_sequence(self, encoder_input: dict, steps: int, beams: int = 1, expand: Optional[int] = None, exclude_seen: bool = True,
                           exclude=None, allow=None, row_filter=None, temperature: float = 1.0, sample_seed: Optional[int] = None,
                           sample_streams=None, return_logp: bool = True):
        """recommend_sequence_tensor as Python lists: per batch row one entry per beam (best first), each an (ids, logp, step_logp)
        tuple -- the path's `steps` ids (-1 where nothing was left), its summed log probability and the log probability of every
        step (None / None where the tensor call returns None)."""
        ids, step_logp, logp, _ = self.recommend_sequence_tensor(encoder_input, steps, beams, expand, exclude_seen, exclude, allow, row_filter,
                                                                 temperature, sample_seed, sample_streams, return_logp)
        ids_h = ids.cpu().tolist()
        step_h = None if step_logp is None else step_logp.cpu().tolist()
        logp_h = None if logp is None else logp.cpu().tolist()
        return [[(ids_h[u][b], None if logp_h is None else logp_h[u][b], None if step_h is None else step_h[u][b])
                 for b in range(len(ids_h[u]))] for u in range(len(ids_h))]

    def explain_tensor(self, encoder_input: Dict[str, torch.Tensor], target_ids, top: int = 3, labels=None, window: Optional[int] = None,
                       exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None,
                       temperature: float = 1.0, rows_per_forward: int = 1024) -> Dict[str, torch.Tensor]:
        """Which history items drove each recommendation, by occlusion: one history unit is removed from the row, the same forward
        runs, and the log probability the explained item loses is the unit's attribution.  The occluded rows are built on the device
        (b4r_occlude_rows, exactly as prepare_inference of the remaining items), their log probabilities come from b4r_score_dist
        with the explained items as its queries, and b4r_attribution_select keeps the `top` units per item.  Nothing is read back
        between the launches.
        encoder_input is prepare_inference's format, as recommend_sequence_tensor takes it; that check is the call's one host
        synchronisation (the largest row length travels back with it, and chunks of units that no row has are skipped).
        target_ids [B, K] int64, 1 <= K <= 1024: the items to explain per batch row, e.g. recommend_tensor's ids; a -1 entry comes
        back dead.  An integer k instead: the row's own top k under the same exclusions and filter, from the same base forward (they
        are returned as target_ids).
        A unit is one history item, counted from the most recent one (w = 0), or with labels [V] int32 (an item's category, -1 = none)
        every history item of one category, which the category's most recent item stands for.  window: only the `window` most recent
        history items are units (None: all L - 1); 1 <= top <= window.
        The counterfactual is taken on the window the model saw: the row as prepared, minus the unit.  An item older than the row's
        L - 1 does not slide back in.  A removed item stays excluded: every distribution of a row has the exclusions of the full row
        (exclude_seen, exclude) and the row's filter (allow, row_filter [B]) at `temperature`, so all of them have the same support,
        the log probabilities are comparable and a finite base_logp has finite occluded ones.
        The units go through the forward in chunks of max(1, rows_per_forward // B) recency indices, B rows each.  The chunking
        regroups the same rows: the result changes only where the encoder forward itself takes another launch form at another row
        count, and then in the last bits of a log probability.
        Returns a dict of device tensors (W = window):
          target_ids     int64 [B, K]
          base_logp      float32 [B, K]: the log probability of each explained item on the row as given (-inf: it cannot be served)
          occluded_logp  float32 [B, W, K]: the same with unit w removed; -inf for a unit the row does not have
          live           int32 [B, W]; unit_pos / unit_label / removed int32 [B, W], unit_item int64 [B, W]: the unit's history
                         position, label (-1 in item mode), the number of items removed and its (most recent) item; -1 / 0 where dead
          top_w, top_pos int32, top_item, top_label int64, top_delta float32 [B, K, top]: the units with the largest base_logp -
                         occluded_logp, best first, ties to the more recent unit; a negative delta (the removal made the item more
                         likely) sorts after the positive ones; -1 / -inf where fewer units are live
          slot_index     int64 [B]: b*P+p, as recommend_tensor returns it."""
        tokens_in = encoder_input.get("input_word_ids") if hasattr(encoder_input, "get") else None
        if tokens_in is None or torch.as_tensor(tokens_in).ndim != 2:
            raise ValueError("explain_tensor takes prepare_inference's batch: input_word_ids [B, L], input_mask and masked_lm_positions")
        B, L = (int(x) for x in torch.as_tensor(tokens_in).shape)
        top, W = engine_mod.check_explain_args(top, window, L, rows_per_forward=rows_per_forward)
        own_k = None
        if isinstance(target_ids, numbers.Integral) and not isinstance(target_ids, bool):
            own_k = K = int(target_ids)
        else:
            target_ids = torch.as_tensor(target_ids)
            if target_ids.ndim != 2 or target_ids.shape[0] != B or target_ids.dtype.is_floating_point or target_ids.dtype == torch.bool:
                raise ValueError(f"target_ids must be an integer tensor [{B}, K], got {target_ids.dtype} of shape {tuple(target_ids.shape)}")
            K = int(target_ids.shape[1])
        engine_mod.check_explain_args(top, W, L, K=K)
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.ndim != 1 or labels.numel() != self.vocab_size or labels.dtype.is_floating_point or labels.dtype == torch.bool:
                raise ValueError(f"labels must hold one integer per item [{self.vocab_size}], got {labels.dtype} of shape {tuple(labels.shape)}")
        engine_mod.check_temperature(temperature)
        allow, rf, (tokens, mask, pos), length, slots0, max_len = self._one_slot_batch("explain_tensor", encoder_input, exclude, allow, row_filter,
                                                                                        max_len=True)
        eng, dev, P = self.engine, self.device, pos.shape[1]
        Wc = min(W, max(1, int(rows_per_forward) // max(B, 1)))
        n_chunks = -(-W // Wc)
        n_run = min(n_chunks, -(-max(max_len - 1, 0) // Wc))       # chunks that start inside the longest history
        ninf = float("-inf")
        out = {"occluded_logp": torch.full((B, n_chunks * Wc, K), ninf, dtype=torch.float32, device=dev),
               "live": torch.zeros((B, n_chunks * Wc), dtype=torch.int32, device=dev),
               "unit_pos": torch.full((B, n_chunks * Wc), -1, dtype=torch.int32, device=dev),
               "unit_item": torch.full((B, n_chunks * Wc), -1, dtype=torch.int64, device=dev),
               "unit_label": torch.full((B, n_chunks * Wc), -1, dtype=torch.int32, device=dev),
               "removed": torch.zeros((B, n_chunks * Wc), dtype=torch.int32, device=dev)}
        first = engine_mod.SPECIAL_IDS
        if B == 0:
            target = torch.empty((0, K), dtype=torch.int64, device=dev)
            base = torch.empty((0, K), dtype=torch.float32, device=dev)
            ex0 = None
        else:
            hidden, _, _ = self._ranked_slot_hidden({"input_word_ids": tokens, "input_mask": mask, "masked_lm_positions": pos}, slots=slots0)
            ex0 = self._excluded_rows(encoder_input, slots0, exclude_seen, exclude)
            if own_k is not None:
                target, _, _ = eng.rank_full(hidden, None, ex0, first, None, own_k, allow, rf)
            else:
                target = target_ids.to(device=dev, dtype=torch.int64).contiguous()
            base = eng.score_distribution(hidden, None, ex0, first, None, allow, rf, temperature, target)[4]
        if B > 0 and n_run > 0:
            N = B * Wc
            st = eng.explain_state(N, L, P)
            len32 = length.to(torch.int32)
            labels_d = None if labels is None else labels.to(device=dev, dtype=torch.int32).contiguous()
            q_rep = target.repeat_interleave(Wc, dim=0)            # every occluded row asks for its user's items ...
            ex_rep = None if ex0 is None else ex0.repeat_interleave(Wc, dim=0)   # ... under the exclusions of the user's FULL row
            rf_rep = None if rf is None else rf.repeat_interleave(Wc)
            slots_c = torch.arange(N, dtype=torch.int64, device=dev) * P
            chunk = {"input_word_ids": st["tokens"], "input_mask": st["mask"], "masked_lm_positions": st["positions"]}
            dead = torch.full((), ninf, dtype=torch.float32, device=dev)
            for j in range(n_run):
                eng.occlude_rows(tokens, len32, labels_d, j * Wc, st)
                hidden, _, _ = self._ranked_slot_hidden(chunk, slots=slots_c)
                lp = eng.score_distribution(hidden, None, ex_rep, first, None, allow, rf_rep, temperature, q_rep)[4]
                cols = slice(j * Wc, (j + 1) * Wc)
                live = st["live"].view(B, Wc)
                out["occluded_logp"][:, cols] = torch.where(live[:, :, None] != 0, lp.view(B, Wc, K), dead)
                out["live"][:, cols] = live
                for name in ("unit_pos", "unit_item", "unit_label", "removed"):
                    out[name][:, cols] = st[name].view(B, Wc)
        out = {name: t[:, :W].contiguous() for name, t in out.items()}   # the last chunk may run past the window
        if B > 0:
            top_w, top_delta = eng.attribution_select(base, out["occluded_logp"], out["live"], top)
        else:
            top_w = torch.empty((0, K, top), dtype=torch.int32, device=dev)
            top_delta = torch.empty((0, K, top), dtype=torch.float32, device=dev)
        at = top_w.clamp(min=0).to(torch.int64).reshape(B, K * top)
        none = top_w < 0
        for name, src, dt in (("top_pos", "unit_pos", torch.int32), ("top_item", "unit_item", torch.int64), ("top_label", "unit_label", torch.int64)):
            out[name] = out[src].gather(1, at).reshape(B, K, top).to(dt).masked_fill(none, -1)
        out.update(target_ids=target, base_logp=base, top_w=top_w, top_delta=top_delta, slot_index=slots0)
        return out

    def explain(self, encoder_input: dict, target_ids, top: int = 3, labels=None, window: Optional[int] = None, exclude_seen: bool = True,
                exclude=None, allow=None, row_filter=None, temperature: float = 1.0, rows_per_forward: int = 1024):
        """explain_tensor as Python lists: per batch row one (item id, log probability, reasons) tuple per explained item, reasons =
        [(history item id, label, history position, delta_logp), ...] best first, dead entries dropped."""
        got = self.explain_tensor(encoder_input, target_ids, top, labels, window, exclude_seen, exclude, allow, row_filter, temperature,
                                  rows_per_forward)
        ids, base = got["target_ids"].cpu().tolist(), got["base_logp"].cpu().tolist()
        item, label, where, delta = (got[name].cpu().tolist() for name in ("top_item", "top_label", "top_pos", "top_delta"))
        return [[(ids[b][i], base[b][i], [(item[b][i][t], label[b][i][t], where[b][i][t], delta[b][i][t])
                                          for t in range(len(item[b][i])) if where[b][i][t] >= 0])
                 for i in range(len(ids[b]))] for b in range(len(ids))]

    def audience_tensor(self, encoder_input: Dict[str, torch.Tensor], item_ids, state=None, k: int = 100, user_ids=None,
                        min_probability=None, exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None, allow=None,
                        row_filter=None, temperature: float = 1.0):
        """Given items, which users?  One batch of users is merged into the k most likely users of each of item_ids [Q] (int64 token
        ids): score_distribution_tensor's forward, exclusions (exclude_seen, exclude) and filter (allow, row_filter [B]) at
        `temperature`, with the Q ids as the queries of every row (in chunks of 1024), then b4r_audience_merge of the [B, Q] log
        probabilities into `state`.  Call it once per batch of users and read the state once, after the last batch: it keeps
        O(Q * k) on the device, no [users, items] matrix, and nothing is read back here.
        A user who has seen an item, may not be served it, or an id outside the vocabulary has log probability -inf and is never in
        that item's audience.
        state: None creates one; else what an earlier call returned for the same item_ids and k (ValueError otherwise).  A dict:
          users   int64 [Q, k]: per item the k most likely users, best first, ties to the lower user id; -1 where there are fewer
          logp    float32 [Q, k]: their log probabilities (-inf in the tail)
          reach   int64 [Q]: the users with probability >= min_probability (None: every user who could be served the item)
          demand  int64 [Q]: the sum of the users' probabilities in units of 2^-40, the expected number of takers
          item_ids (host) / query_ids (device) int64 [Q], next_user: the id of the next unnamed row
        The result depends only on the set of (user, log probability) pairs: not on the batches the users came in, nor on their
        order, bit for bit (the log probabilities themselves come from the forward, which may take another launch form at another
        batch size).
        user_ids [B] int64 >= 0 name the batch rows (distinct over all calls); None: state["next_user"] + row, which then advances.
        The batch is prepare_inference's: exactly one ranked slot per row (masked_lm_weights; without them P must be 1)."""
        engine_mod.check_temperature(temperature)
        k, min_logp = engine_mod.check_audience_args(k, min_probability)
        item_ids = engine_mod.check_audience_items(item_ids)
        if state is not None:
            engine_mod.check_audience_state(state, item_ids, k)
        B, P, slot, user_ids, allow, row_filter = self._audience_batch("audience_tensor", encoder_input, user_ids, allow, row_filter)
        if state is None:
            state = self.engine.audience_state(item_ids, k)
        if B == 0:
            return state
        hidden, ex_rows, user_ids, user0 = self._audience_rows(encoder_input, B, P, slot, exclude_seen, exclude, user_ids, state)
        Q = int(item_ids.numel())
        for c0 in range(0, Q, engine_mod.RANK_FULL_MAX_K):
            c1 = min(Q, c0 + engine_mod.RANK_FULL_MAX_K)
            queries = state["query_ids"][c0:c1].unsqueeze(0).expand(B, c1 - c0)
            logp = self.engine.score_distribution(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, allow, row_filter, temperature,
                                                  queries)[4]
            self.engine.audience_merge(logp, state["users"][c0:c1], state["logp"][c0:c1], state["reach"][c0:c1], state["demand"][c0:c1],
                                       user_ids, user0, min_logp)
        return state

    def _audience_batch(self, caller: str, encoder_input, user_ids, allow, row_filter):
        """The checks of an audience batch that need no forward: prepare_inference's format with exactly one ranked slot per row,
        user_ids [B], allow / row_filter.  Returns (B, P, the ranked slot of every row [B] int64 on the host side of the weights,
        user_ids int64 [B] or None, packed allow or None, row_filter or None)."""
        tokens_in = encoder_input.get("input_word_ids") if hasattr(encoder_input, "get") else None
        positions = encoder_input.get("masked_lm_positions") if tokens_in is not None else None
        if tokens_in is None or positions is None or torch.as_tensor(tokens_in).ndim != 2 or torch.as_tensor(positions).ndim != 2:
            raise ValueError(f"{caller} takes prepare_inference's batch: input_word_ids [B, L] and masked_lm_positions [B, P]")
        B, P = int(torch.as_tensor(tokens_in).shape[0]), int(torch.as_tensor(positions).shape[1])
        weights = encoder_input.get("masked_lm_weights")
        if weights is None:
            if P != 1:
                raise ValueError(f"an audience batch has exactly one ranked slot per row: without masked_lm_weights P must be 1, got {P}")
            slot = torch.zeros((B,), dtype=torch.int64)
        else:
            w = torch.as_tensor(weights).reshape(B, P) != 0          # checked where the tensor lives: a host batch costs no device sync
            if not bool((w.sum(dim=1) == 1).all()):
                raise ValueError("an audience batch has exactly one ranked slot per row (prepare_inference's format)")
            slot = w.to(torch.int64).argmax(dim=1)
        if user_ids is not None:
            user_ids = engine_mod.check_sample_streams(user_ids, B)   # [B] integers -> int64
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        return B, P, slot, user_ids, allow, row_filter

    def _audience_rows(self, encoder_input, B: int, P: int, slot: torch.Tensor, exclude_seen: bool, exclude, user_ids, state,
                       forward_rows: Optional[int] = None):
        """The forward of an audience batch (B >= 1) and the names of its rows.  Returns (hidden [B, H], exclude rows or None,
        user_ids on the device or None, user0: the id of row 0 when the rows are unnamed; state["next_user"] then advances).
        forward_rows: None = one forward over the batch as it comes; else _hidden_in_blocks of that many rows, placed by user id."""
        dev = self.device
        slots = torch.arange(B, dtype=torch.int64, device=dev) * P + slot.to(dev)
        if forward_rows is None:
            hidden, slots, _ = self._ranked_slot_hidden(encoder_input, slots=slots)
        else:
            users = user_ids.cpu() if user_ids is not None else int(state["next_user"]) + torch.arange(B, dtype=torch.int64)
            hidden = self._hidden_in_blocks(encoder_input, B, P, slot, forward_rows, users)
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        user0 = 0
        if user_ids is None:
            user0 = int(state["next_user"])
            state["next_user"] = user0 + B
        else:
            user_ids = user_ids.to(dev).contiguous()
        return hidden, ex_rows, user_ids, user0

    # ---- category affinity --------------------------------------------------------------------------------------------------
    def _group_affinity(self, hidden, ex_rows, labels_d: torch.Tensor, G: int, allow, row_filter, temperature):
        """One b4r_score_dist sweep for the rows' normalisers and one b4r_group_mass: group_affinity_tensor's dict without slot_index."""
        n, _, lse, _, _ = self.engine.score_distribution(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, None, allow, row_filter, temperature)
        mass, gn, rest_mass, rest_n = self.engine.group_mass(hidden, None, ex_rows, engine_mod.SPECIAL_IDS, lse, labels_d, G, allow,
                                                             row_filter, temperature)
        logp = torch.log(mass.to(torch.float64) * (1.0 / engine_mod.GROUP_MASS_ONE)).to(torch.float32)   # log(0) = -inf
        return {"group_mass": mass, "group_n": gn, "group_logp": logp, "rest_mass": rest_mass, "rest_n": rest_n, "row_lse": lse,
                "row_n": n}

    def group_affinity_tensor(self, encoder_input: Dict[str, torch.Tensor], item_groups, n_groups=None, exclude_seen: bool = True,
                              exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None, temperature: float = 1.0):
        """P(next item in group g | user) for every ranked slot and every item group: the sum of the catalogue softmax over the items
        of the group the slot could be served -- score_distribution_tensor's forward, exclusions, filter and temperature -- from one
        b4r_score_dist sweep (the normalisers) and one b4r_group_mass sweep: no [R, V] probabilities anywhere.
        item_groups: int32 / int64 [V], one label per token id, negative = no group; n_groups: None = the largest label + 1, at most
        65536; a label >= n_groups counts as no group (engine.check_item_group_labels).  Returns a dict of device tensors:
          group_mass  int64 [R, G]: the mass of each group in units of 2^-40 (engine.GROUP_MASS_ONE = probability 1), an integer sum
                      of the items' rounded probabilities: it does not depend on the order of the rows or on the batching
          group_n     int32 [R, G]: the items of the group the slot could be served
          group_logp  float32 [R, G]: fl32(log(group_mass * 2^-40)), -inf where the mass is 0
          rest_mass / rest_n  int64 / int32 [R]: the same for the items without a group; sum(group_n) + rest_n = row_n
          row_lse     float64 [R], row_n int32 [R]: score_distribution_tensor's lse and n
          slot_index  int64 [R]: b*P+p, as recommend_tensor returns it
        Resolution: one unit is 2^-40 (9.1e-13).  Every item's probability is rounded to a whole number of units, so a mass is off by
        up to half a unit per item of the group: a group whose mass is below about 1e-9 holds few units, and a group whose items all
        lie below 2^-41 reads 0 (group_logp = -inf) while group_n > 0."""
        engine_mod.check_temperature(temperature)
        labels, G = engine_mod.check_item_group_labels(item_groups, self.vocab_size, n_groups)
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        dev = self.device
        if hidden is None:
            z = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)
            return {"group_mass": z(torch.int64, 0, G), "group_n": z(torch.int32, 0, G), "group_logp": z(torch.float32, 0, G),
                    "rest_mass": z(torch.int64, 0), "rest_n": z(torch.int32, 0), "row_lse": z(torch.float64, 0),
                    "row_n": z(torch.int32, 0), "slot_index": slots}
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        out = self._group_affinity(hidden, ex_rows, labels.to(dev), G, allow, row_filter, temperature)
        out["slot_index"] = slots
        return out

    def recommend_shelves_tensor(self, encoder_input: Dict[str, torch.Tensor], item_groups, n_groups=None, shelves: int = 3, k: int = 10,
                                 exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None, allow=None,
                                 temperature: float = 1.0):
        """A page of shelves for every ranked slot: the `shelves` item groups with the largest affinity ("Top in Horror" before "Top in
        Comedy" for this user), each with its k best items.  A composition: group_affinity_tensor's two sweeps, the choice of the
        groups on the device (mass descending, ties to the lower group; a group with group_n = 0 is never a shelf), and ONE
        b4r_rank_full_ex call over the R * shelves rows, each pointing at its slot's hidden row and at its group's item filter
        (engine.pack_group_filters, built once per call).  allow: None or one bool / uint8 mask [V] for all rows.  At most 1024 groups.
        Returns (shelf_group [R, shelves] int64: the group of each shelf, -1 where the slot has fewer groups to be served from;
        shelf_mass [R, shelves] int64 in units of 2^-40; ids [R, shelves, k] int64 and scores [R, shelves, k] fp32: b4r_rank_full's
        within the group, -1 / -inf in the tail; slot_index [R]), on the device: nothing is read back here."""
        engine_mod.check_temperature(temperature)
        labels, G = engine_mod.check_item_group_labels(item_groups, self.vocab_size, n_groups)
        shelves, k = engine_mod.check_shelf_args(shelves, k, G)
        if allow is not None:
            allow = torch.as_tensor(allow)
            if allow.dtype not in (torch.bool, torch.uint8) or tuple(allow.shape) != (self.vocab_size,):
                raise ValueError(f"allow is one bool / uint8 mask [{self.vocab_size}] here, got {allow.dtype} of shape {tuple(allow.shape)}")
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        dev = self.device
        R = int(slots.numel())
        if hidden is None:
            return (torch.empty((0, shelves), dtype=torch.int64, device=dev), torch.empty((0, shelves), dtype=torch.int64, device=dev),
                    torch.empty((0, shelves, k), dtype=torch.int64, device=dev), torch.empty((0, shelves, k), dtype=torch.float32, device=dev),
                    slots)
        labels_d = labels.to(dev)
        filters = engine_mod.pack_group_filters(labels_d, G, None if allow is None else allow.to(dev))   # [G + 1, W]: built once
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        aff = self._group_affinity(hidden, ex_rows, labels_d, G, None if allow is None else allow, None, temperature)
        key = torch.where(aff["group_n"] > 0, aff["group_mass"], torch.full_like(aff["group_mass"], -1))
        mass, group = torch.sort(key, dim=1, descending=True, stable=True)       # ties keep the lower group first
        mass, group = mass[:, :shelves], group[:, :shelves]
        group = torch.where(mass >= 0, group, torch.full_like(group, -1))
        rows = torch.arange(R, dtype=torch.int64, device=dev).repeat_interleave(shelves)
        row_filter = torch.where(group >= 0, group, torch.full_like(group, G)).reshape(-1).to(torch.int32)   # G: the empty filter
        ex = None if ex_rows is None else ex_rows.repeat_interleave(shelves, dim=0)
        ids, scores, _ = self.engine.rank_full(hidden, rows, ex, engine_mod.SPECIAL_IDS, None, k, filters, row_filter)
        return group, mass.clamp(min=0), ids.reshape(R, shelves, k), scores.reshape(R, shelves, k), slots

    def _hidden_in_blocks(self, encoder_input, B: int, P: int, slot: torch.Tensor, block: int, users: torch.Tensor) -> torch.Tensor:
        """_ranked_slot_hidden of a one-slot-per-row batch whose rows are named by users [B] (int64, host), such that a user's hidden
        state has the same bits in whatever batch the user comes.  Two things stand in the way otherwise: the
        encoder takes another launch form at another row count, and in the hidden-64 kernels, which work on tiles of 32 rows, a row's
        last bits follow its place in the tile.  So the forward runs on blocks of exactly `block` rows and user u always sits at
        place u mod block of a block (rows that share a place go to successive blocks; the empty places hold copies of row 0, which
        are dropped).  What a row shares its block with does not matter.  Consecutive ids fill the blocks without gaps.
        Returns hidden [B, H]."""
        dev = self.device
        tensors = {key: torch.as_tensor(v) for key, v in encoder_input.items() if v is not None}
        place = torch.remainder(users, block)
        order = torch.argsort(place, stable=True)
        run_start = torch.searchsorted(place[order], place[order])           # where the rows of the same place begin, in that order
        nth = torch.empty(B, dtype=torch.int64)
        nth[order] = torch.arange(B) - run_start                             # row r is the nth[r]-th of its place, in row order
        at = nth * block + place
        n_blocks = int(nth.max()) + 1
        src = torch.zeros(n_blocks * block, dtype=torch.int64)
        src[at] = torch.arange(B)
        parts = []
        for j in range(n_blocks):
            idx = src[j * block:(j + 1) * block]
            part = {key: v[idx.to(v.device)] if v.ndim >= 1 and v.shape[0] == B else v for key, v in tensors.items()}
            slots = torch.arange(block, dtype=torch.int64, device=dev) * P + slot[idx.to(slot.device)].to(dev)
            hidden, _, _ = self._ranked_slot_hidden(part, slots=slots)
            parts.append(hidden.clone())                   # (the next block's forward reuses the buffers)
        return torch.cat(parts, dim=0)[at.to(dev)]

    def group_audience_tensor(self, encoder_input: Dict[str, torch.Tensor], item_groups, n_groups, state=None, k: int = 100, user_ids=None,
                              min_probability=None, exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None, allow=None,
                              row_filter=None, temperature: float = 1.0, forward_rows: Optional[int] = 256):
        """Given item groups, which users?  audience_tensor with the G groups in place of the Q items: one batch of users is merged
        into the k users most likely to take an item of each group next.  group_affinity_tensor's group_logp [B, G] goes straight into
        b4r_audience_merge.  state: None creates one; else what an earlier call returned for the same n_groups and k.  The dict is
        audience_tensor's (users, logp [G, k]; reach, demand [G]; item_ids holds the group indices 0 .. G-1), plus "labels": the
        labels on the device, uploaded once.  Later calls must bring the same item_groups.
        The state depends only on the set of (user, group_logp) pairs, and group_logp comes from integer sums over a fixed-order
        normaliser: given a user's hidden state it does not depend on the batch the user came in.
        forward_rows (default 256): the encoder runs on blocks of exactly that many rows with user u at place u mod forward_rows of
        its block (the places left empty hold copies of a row), so that it takes the same launch form at every batch size and a row
        keeps its place in the kernels' row tiles: a user's hidden state does not depend on the batch either.  The state is then the
        same in every bit however the users are cut into calls and in whatever order the calls arrive; the price is the padding (a
        call with one user costs a forward of forward_rows; consecutive ids fill the blocks without gaps) and a host copy of
        user_ids.  None: one forward over the batch as it comes, audience_tensor's way: the same batches in another order give the
        same bits, other batch sizes may differ in a log probability's last bits.
        A user who can be served nothing of a group has -inf there and is never in that group's audience.  demand [G] sums
        llrint(exp(group_logp) * 2^40) over the users: the expected number of users whose next item is of the group."""
        engine_mod.check_temperature(temperature)
        k, min_logp = engine_mod.check_audience_args(k, min_probability)
        if forward_rows is not None:
            forward_rows = engine_mod._int_in(forward_rows, 1, 1 << 20, "forward_rows")
        if n_groups is None:
            raise ValueError("n_groups names the groups of the state: give it")
        if state is None or state.get("labels") is None:
            labels, G = engine_mod.check_item_group_labels(item_groups, self.vocab_size, n_groups)
        else:
            labels, G = None, engine_mod._int_in(n_groups, 1, engine_mod.GROUP_MASS_MAX_G, "n_groups")
        group_ids = torch.arange(G, dtype=torch.int64)
        if state is not None:
            engine_mod.check_audience_state(state, group_ids, k)
        B, P, slot, user_ids, allow, row_filter = self._audience_batch("group_audience_tensor", encoder_input, user_ids, allow, row_filter)
        if state is None:
            state = self.engine.audience_state(group_ids, k)
        if state.get("labels") is None:
            state["labels"] = labels.to(self.device)
        if B == 0:
            return state
        hidden, ex_rows, user_ids, user0 = self._audience_rows(encoder_input, B, P, slot, exclude_seen, exclude, user_ids, state,
                                                               forward_rows)
        logp = self._group_affinity(hidden, ex_rows, state["labels"], G, allow, row_filter, temperature)["group_logp"]
        self.engine.audience_merge(logp, state["users"], state["logp"], state["reach"], state["demand"], user_ids, user0, min_logp)
        return state

    def recommend_joint_tensor(self, encoder_input: Dict[str, torch.Tensor], parties, k: int = 10, strategy: str = "additive", weights=None,
                               min_member_probability=None, calibrated: bool = True, exclude_seen: bool = True,
                               exclude: Optional[torch.Tensor] = None, allow=None, row_filter=None, temperature: float = 1.0,
                               return_members: bool = False):
        """Several users deciding together: one top-k list of the whole catalogue per PARTY of batch rows (a household, friends, a
        shared playlist), from one b4r_rank_joint sweep: no [B, V] scores.  parties [NP, M] integers, M <= 16: the batch rows of each
        party, -1 padded; a row may belong to several parties.  An item is ranked for a party when every member could be served it
        (recommend_tensor's exclusions -- exclude_seen, exclude -- and filter -- allow, row_filter [B] -- per member: an item any
        member has seen is out).  strategy, over the members' scores of the item:
          "additive"       their sum, each times its entry of weights [NP, M] (None: 1)
          "least_misery"   their minimum: nobody is left with an item they dislike
          "most_pleasure"  their maximum
        calibrated (default): a member's score is the log probability of the item under the member's catalogue softmax at
        `temperature` (score_distribution_tensor's logp: one b4r_score_dist sweep for the normalisers first), which is what makes the
        scores of different users comparable; the additive aggregate is then the log of the product of the probabilities.
        min_member_probability q in (0, 1]: the veto -- an item some member takes with probability below q is out.
        calibrated=False skips the distribution sweep and aggregates the raw scores (min_member_probability must be None, temperature
        1).  Returns device tensors (ids [NP,k] int64, scores [NP,k] fp32: the aggregates, descending, ties to the lower id, n [NP]
        int32: the items the party could be served), -1 / -inf where there are fewer than k; with return_members a fourth,
        member_logp [NP,k,M] fp32: each member's own score of each returned item (-inf for an absent slot and under the -1 tail).
        A party without members, or with a member who can be served nothing, gets an empty list.
        The batch is prepare_inference's: exactly one ranked slot per row."""
        rows_in = encoder_input.get("input_word_ids") if hasattr(encoder_input, "get") else None
        if rows_in is None or torch.as_tensor(rows_in).ndim != 2:
            raise ValueError("recommend_joint_tensor takes prepare_inference's batch: input_word_ids [B, L] and masked_lm_positions [B, P]")
        B = int(torch.as_tensor(rows_in).shape[0])
        parties, k, _, w, min_util, _ = engine_mod.check_joint_args(parties, k, strategy, weights, min_member_probability, calibrated,
                                                                    temperature, B)
        allow, rf, (tokens, mask, pos), _, slots, _ = self._one_slot_batch("recommend_joint_tensor", encoder_input, exclude, allow, row_filter)
        NP, M = (int(x) for x in parties.shape)
        dev, first = self.device, engine_mod.SPECIAL_IDS
        if B == 0 or NP == 0:
            out = (torch.full((NP, k), -1, dtype=torch.int64, device=dev), torch.full((NP, k), float("-inf"), dtype=torch.float32, device=dev),
                   torch.zeros((NP,), dtype=torch.int32, device=dev))
            return out + (torch.full((NP, k, M), float("-inf"), dtype=torch.float32, device=dev),) if return_members else out
        hidden, _, _ = self._ranked_slot_hidden({"input_word_ids": tokens, "input_mask": mask, "masked_lm_positions": pos}, slots=slots)
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        lse = self.engine.score_distribution(hidden, None, ex_rows, first, None, allow, rf, temperature)[2] if calibrated else None
        ids, scores, n, util = self.engine.rank_joint(hidden, None, ex_rows, first, parties, k, strategy, w, min_util, lse, allow, rf,
                                                      temperature, return_members)
        return (ids, scores, n, util) if return_members else (ids, scores, n)

    def recommend_joint(self, encoder_input: dict, parties, k: int = 10, strategy: str = "additive", weights=None,
                        min_member_probability=None, calibrated: bool = True, exclude_seen: bool = True, exclude=None, allow=None,
                        row_filter=None, temperature: float = 1.0, return_members: bool = False):
        """recommend_joint_tensor as Python lists: per party (ids, scores, n), or (ids, scores, n, member_logp) with return_members;
        ids and scores have length k (-1 / -inf where the party could be served fewer)."""
        got = self.recommend_joint_tensor(encoder_input, parties, k, strategy, weights, min_member_probability, calibrated, exclude_seen,
                                          exclude, allow, row_filter, temperature, return_members)
        cols = [t.cpu().tolist() for t in got]
        return [tuple(col[p] for col in cols) for p in range(len(cols[0]))]

    def allocate_tensor(self, encoder_input: Dict[str, torch.Tensor], capacity, k: int = 10, pool: Optional[int] = None,
                        calibrated: bool = True, user_ids=None, exclude_seen: bool = True, exclude: Optional[torch.Tensor] = None,
                        allow=None, row_filter=None, temperature: float = 1.0, max_rounds: Optional[int] = None):
        """Stock-aware recommendations: at most k items for every ranked slot, with every item handed out at most capacity[item]
        times over the whole batch (coupons, one-off listings, seats, "this campaign reaches at most c users").  capacity: one
        integer per token id [V], the units on offer (<= 0: none; engine.ALLOCATE_UNLIMITED = 2^31 - 1 for an item without a limit).
        One forward (recommend_tensor's: the same slots, exclusions and filter), one b4r_rank_full sweep for the best `pool` allowed
        items of every slot (default min(1024, max(10 k, 50)), the re-rankers'), then b4r_allocate over the pools on the device.
        calibrated (default): the utility of a pool entry is its log probability under the slot's catalogue softmax at `temperature`
        (one b4r_score_dist sweep with the pool ids as the queries), which is what makes the utilities of different users
        comparable, as in recommend_joint_tensor; calibrated=False uses the raw sweep scores (temperature must be 1).
        The entries of all slots are walked in one order -- utility descending, then the lower user_ids entry ([R] integers, one per
        ranked slot; None: the slot's row number 0 .. R-1), the lower row, the lower pool position -- and an entry is given to its
        slot while the slot holds fewer than k and the item has units left: a contended item goes to the users who want it most, and
        a user who loses it gets the next item of their own pool instead.
        Returns (ids [R,k] int64, util [R,k] fp32, slot_index [R] int64 = b*P+p, info), on the device; every slot's items stand in
        its pool's order (best first), -1 / -inf behind them when the pool, under the stock, yields fewer than k.  info: pos [R,k]
        int32 (the pool position of every item), row_n [R] int32 (the items the slot got), remaining [V] int32 (capacity minus what
        was given: the capacity of the next batch, first come, first served -- the result depends on how users are cut into batches),
        unsettled (one int32: 0 = the lists are final).  max_rounds=None settles the allocation (a 4-byte read-back per 32 rounds);
        an integer enqueues exactly that many rounds without a synchronisation (Engine.allocate)."""
        k = engine_mod.check_rank_full_args(k, exclude)
        k, n_sweep, _ = engine_mod.check_rerank_args(k, pool, 0.0)
        if not calibrated and not (isinstance(temperature, numbers.Real) and temperature == 1.0):
            raise ValueError("temperature scales the calibrated utilities: calibrated=False takes temperature 1")
        engine_mod.check_temperature(temperature)
        cap = engine_mod.check_capacity(capacity, self.vocab_size)
        allow, row_filter = engine_mod.check_item_filter(allow, row_filter, self.vocab_size)
        hidden, slots, _ = self._ranked_slot_hidden(encoder_input)
        R = int(slots.numel())
        engine_mod.check_allocate_args(k, R, n_sweep, max_rounds)
        uid = engine_mod.check_allocate_user_ids(user_ids, R)
        dev, first = self.device, engine_mod.SPECIAL_IDS
        if hidden is None:
            info = {"pos": torch.empty((0, k), dtype=torch.int32, device=dev), "row_n": torch.empty((0,), dtype=torch.int32, device=dev),
                    "remaining": cap.to(dev), "unsettled": torch.zeros((1,), dtype=torch.int32, device=dev)}
            return torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev), slots, info
        ex_rows = self._excluded_rows(encoder_input, slots, exclude_seen, exclude)
        pool_ids, pool_util, _ = self.engine.rank_full(hidden, None, ex_rows, first, None, n_sweep, allow, row_filter)
        if calibrated:
            pool_util = self.engine.score_distribution(hidden, None, ex_rows, first, None, allow, row_filter, temperature, pool_ids)[4]
        ids, util, pos, row_n, remaining, unsettled = self.engine.allocate(pool_ids, pool_util, k, cap, uid, max_rounds)
        return ids, util, slots, {"pos": pos, "row_n": row_n, "remaining": remaining, "unsettled": unsettled}

    def _rank_items_ragged(self, encoder_input, items):
        """Candidate lists of different lengths: one kernel call per distinct length."""
        flat = [c for row in items for c in row]
        hidden, slots, counts = self._ranked_slot_hidden(encoder_input)
        if len(flat) != int(slots.numel()):
            raise ValueError(f"{len(flat)} candidate lists for {int(slots.numel())} masked slots")
        results: List[Optional[torch.Tensor]] = [None] * len(flat)
        for n in sorted({len(c) for c in flat}):
            idx = [i for i, c in enumerate(flat) if len(c) == n]
            cand = torch.tensor([flat[i] for i in idx], dtype=torch.int64)
            ranking, _, _ = self.engine.rank_candidates(hidden, torch.tensor(idx, dtype=torch.int64), cand, None)
            for j, i in enumerate(idx):
                results[i] = ranking[j]
        out, r = [], 0
        for n in counts:
            out.append(results[r:r + n])
            r += n
        return out

    # ---- weights ----------------------------------------------------------------------------------------------------------
    @property
    def trainable_variables(self) -> List[str]:
        return [e.name for e in self.engine.table]

    def get_weights(self) -> Dict[str, torch.Tensor]:
        """Variables under the reference's Keras names and shapes (CPU tensors)."""
        return self.engine.export_named()

    def set_weights(self, weights: Dict[str, torch.Tensor]) -> None:
        e = self.engine
        table = weights.get("word_embeddings/embeddings")
        if table is not None and tuple(table.shape)[-1] != e.embedding_width:
            raise ValueError(f"the checkpoint's item table is {tuple(table.shape)} wide, the model's embedding_width is "
                             f"{e.embedding_width}: build the encoder with embedding_width={tuple(table.shape)[-1]}")
        if ("embedding_projection/kernel" in weights) != e.factorised:
            raise ValueError("the checkpoint %s embedding_projection/* but the model is %s" %
                             ("has" if "embedding_projection/kernel" in weights else "lacks",
                              "factorised" if e.factorised else "not factorised"))
        e.load_named(weights)

    def save_weights(self, filepath) -> None:
        from safetensors.torch import save_file
        w = {k: v.contiguous() for k, v in self.get_weights().items()}
        save_file(w, str(filepath), metadata={"format": "bert4rec_amd", "model": self.name})

    def load_weights(self, filepath) -> None:
        """Weights only: like the reference's resume path the optimizer state is NOT restored (bert4rec_trainer.py:53-58)."""
        from safetensors.torch import load_file
        self.set_weights(load_file(str(filepath)))

    def get_config(self):
        return dict(self._config)

    @classmethod
    def from_config(cls, config, custom_object=None):
        return cls(**config)


def _dp_rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:   # pragma: no cover
        pass
    return 0, 1


def dp_shard(batches, rank: int, world: int):
    """The batches rank `rank` of `world` trains on in one epoch, one entry per ROUND (= per all-reduce): batch
    round * world + rank, or None where the last round has no batch left for this rank.  Every rank sees the same number of
    rounds, and EVERY batch is consumed by exactly one rank: a rank without a batch joins the round's all-reduce with zero
    gradients and zero sums (Engine.dp_idle_step), which is the reference's single-process step on the batches that are there
    (trainer_utils.py:19-22 normalises by the count of valid slots).  Round 3 dropped the trailing len % world batches -- with the
    reference's default reshuffle_each_iteration=False (dataloader_utils.py:306-311) the SAME batches were then never trained on.
    world == 1: all of them."""
    if world <= 1:
        yield from batches
        return
    n = len(batches)
    mine = iter(b for i, b in enumerate(batches) if i % world == rank)
    for r in range(-(-n // world)):
        yield next(mine) if r * world + rank < n else None
