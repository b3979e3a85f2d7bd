"""Single-sequence recommendation (the reference's demo app, bert4rec/apps/recommender.py:14-63): append a masked slot to the
history (prepare_inference), score the whole vocabulary for that slot and return the best item(s) the user has not seen.

On the GPU this is the evaluation path: encoder forward, tfm MaskedLM's transform on the ONE masked slot, one
b4r_rank_candidates call over the whole vocabulary (cand = NULL: no [1, V] candidate list, no [B, P, V] logits).  Deliberate
differences from the reference, both documented in INTEGRATION.md: it reads ``mlm_logits[:, -1]``, i.e. the LAST of the P slots
-- a padded slot that gathers position 0 -- where the masked token sits in slot 0 (used here); and it can return [PAD] / [MASK] /
[UNK], which are excluded here together with the seen items.

recommend_batch serves many users at once: one forward over the stacked batch and one b4r_rank_full call (the best k allowed items of
every user in one sweep over the vocabulary, no [users, V] scores, the seen items excluded on the device).

allowed_items / allowed_items_per_user restrict the catalogue (items in stock, one category, one allow-list per market): the lists
become packed item filters that the same sweep applies (b4r_rank_full_ex).  similar_items returns the nearest neighbours of items in
the learned item table (b4r_item_neighbours).

diversity (0 = the plain top k, the default; up to 1) trades relevance against similarity among the returned items: the sweep returns
candidate_pool candidates per user and b4r_rerank_diverse picks k of them by greedy Maximal Marginal Relevance, cosine in the item table.

max_per_group caps how many of the returned items may share a category / brand / artist: the sweep returns candidate_pool candidates
per user and b4r_rerank_quota picks k of them under the caps, in relevance order (or by MMR when diversity is given as well).

return_probabilities / min_probability / temperature turn the scores into probabilities over the catalogue each user could have been
served (b4r_score_dist: one more sweep, no [users, V] scores): every recommended item comes with its probability, and items below a
threshold are dropped.

list_quality measures what such lists are like beyond accuracy (b4r_list_metrics): intra-list diversity, catalogue coverage, novelty.

explain_batch / explain say why an item is recommended ("because you watched X"): one history item, or every history item of one
category, is removed at a time on the device (b4r_occlude_rows), the model runs again, and the history items whose removal costs the
recommendation the most log probability come back as its reasons (b4r_attribution_select).

audience turns the question round: given items, which users?  The users go through the model in batches, and the k most likely users
of every item, its reach and its expected demand are kept on the device while the batches go by (b4r_audience_merge).

category_affinity gives each user's probability of picking from every category next (b4r_group_mass: the catalogue softmax summed
per item group on the device, no [users, V] probabilities); category_audience is `audience` with categories in place of items, and
recommend_shelves returns the categories a user is most likely to pick from, each with its best items.

calibrate_by / calibrate_to / calibration give every user a list with their own category mix: the sweep returns candidate_pool
candidates per user and b4r_rerank_calibrated picks k of them so that the list's category shares follow the shares of the user's
history, or the user's category affinity.

allocate shares limited items out among the users of one call (a stock of coupons, listings that exist once, seats): no item is handed
out more often than its stock, a contended item goes to the users most likely to take it, and whoever loses it gets the next item of
their own pool (b4r_allocate over the users' candidate pools, which stay on the device)."""
import numbers

import numpy as np
import torch

from .. import engine as engine_mod
from ..engine import SPECIAL_IDS, _as_cap, item_self_information, pack_item_groups


class Recommender:
    def __init__(self, model, dataloader):
        self.model = model
        self.dataloader = dataloader

    def _known_tokens(self, items) -> list:
        """Token ids of the items the vocabulary knows, in order; unknown items are ignored (and never added to the vocabulary)."""
        tokenizer = self.dataloader.get_tokenizer()
        extensible = getattr(tokenizer, "_extensible", False)
        tokenizer.disable_extensibility()
        tokens = []
        try:
            for item in items:
                try:
                    t = tokenizer.tokenize(item)
                except (RuntimeError, ValueError):
                    continue
                if isinstance(t, int) and 0 <= t < self.model.vocab_size:
                    tokens.append(t)
        finally:
            if extensible:
                tokenizer.enable_extensibility()
        return tokens

    def _item_mask(self, items) -> torch.Tensor:
        mask = torch.zeros(self.model.vocab_size, dtype=torch.bool)
        tokens = self._known_tokens(items)
        if tokens:
            mask[torch.as_tensor(tokens, dtype=torch.int64)] = True
        return mask

    def _token_ids(self, items) -> torch.Tensor:
        """The token id of every item, int64 [len(items)]; -1 for an item the vocabulary does not know."""
        ids = torch.full((len(items),), -1, dtype=torch.int64)
        for j, item in enumerate(items):
            t = self._known_tokens([item])
            if t:
                ids[j] = t[0]
        return ids

    @staticmethod
    def _padded_ids(token_lists) -> torch.Tensor:
        """Lists of token ids as one int64 matrix, -1 padded to the longest list (at least one column)."""
        ids = torch.full((len(token_lists), max(1, max(len(t) for t in token_lists))), -1, dtype=torch.int64)
        for i, t in enumerate(token_lists):
            if t:
                ids[i, :len(t)] = torch.as_tensor(t, dtype=torch.int64)
        return ids

    def _requests(self, sequences):
        """One request per sequence: (prepare_inference's batches stacked into one, exclude [n, longest] int64: every item of the
        sequence, also those before the model's window, -1 padded)."""
        batches = [self.dataloader.prepare_inference(list(seq)) for seq in sequences]
        batch = {key: torch.from_numpy(np.concatenate([np.asarray(b[key]) for b in batches], axis=0)) for key in batches[0]}
        return batch, self._padded_ids([self.dataloader.get_tokenizer().tokenize(seq) for seq in sequences])

    def _allow_filters(self, n_sequences: int, allowed_items, allowed_items_per_user):
        """allowed_items (one iterable of items for all users) or allowed_items_per_user (one per sequence; lists with the same known
        items share one filter) -> (allow: a bool mask [V], masks [F, V] or None; the filter index of every sequence int32 [n] or
        None).  The argument errors come before the tokenizer is touched."""
        if allowed_items is not None and allowed_items_per_user is not None:
            raise ValueError("give allowed_items or allowed_items_per_user, not both")
        if allowed_items is not None:
            return self._item_mask(allowed_items), None
        if allowed_items_per_user is None:
            return None, None
        lists = [list(items) for items in allowed_items_per_user]
        if len(lists) != n_sequences:
            raise ValueError(f"{len(lists)} allow-lists for {n_sequences} sequences")
        distinct = {}
        user_filter = [distinct.setdefault(frozenset(self._known_tokens(items)), len(distinct)) for items in lists]
        allow = torch.zeros((max(len(distinct), 1), self.model.vocab_size), dtype=torch.bool)
        for tokens, f in distinct.items():
            if tokens:
                allow[f, torch.as_tensor(sorted(tokens), dtype=torch.int64)] = True
        return allow, torch.as_tensor(user_filter, dtype=torch.int32)

    def _label_tokens(self, look, catalogue=None):
        """look(item) = the item's hashable group label or None, asked for every item of the vocabulary -> (the group index of every
        token id, int64 [V] with -1 = no group; {label: group index} in order of first appearance).  catalogue: the (token, item)
        pairs, for a caller that labels them more than once."""
        index, groups = {}, np.full(self.model.vocab_size, -1, dtype=np.int64)
        for t, item in catalogue or self._catalogue():
            label = look(item)
            if label is not None:
                groups[t] = index.setdefault(label, len(index))
        return groups, index

    def _catalogue(self) -> list:
        tokens = list(range(SPECIAL_IDS, self.model.vocab_size))
        return list(zip(tokens, self.dataloader.get_tokenizer().detokenize(tokens)))

    def _item_groups(self, max_per_group) -> list:
        """(labels, cap) or a list of such pairs -> pack_item_groups specs, through the tokenizer.  labels: a mapping (or a callable)
        from a detokenized item to a hashable group label; an item it does not know, or maps to None, is in no group.  cap: one int
        for every group, or a mapping label -> int (a label it does not hold is not capped).  The specs are packed for this one call
        and live on the model's device, so nothing of them outlives the call."""
        pairs = [max_per_group] if isinstance(max_per_group, tuple) and len(max_per_group) == 2 and \
            not isinstance(max_per_group[0], tuple) else list(max_per_group)
        catalogue = self._catalogue()
        specs = []
        for pair in pairs:
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("max_per_group takes (labels, cap) or a list of such pairs")
            labels, cap = pair
            look = labels if callable(labels) else getattr(labels, "get", None)   # (a callable's own errors are the caller's to see)
            if look is None:
                raise ValueError("labels maps an item to its group label: a mapping or a callable")
            groups, index = self._label_tokens(look, catalogue)
            if hasattr(cap, "get"):
                big = (1 << 31) - 1
                caps = np.full(len(index), big, dtype=np.int64)
                for label, g in index.items():
                    c = cap.get(label)
                    if c is not None:
                        caps[g] = _as_cap(c, f"the cap of {label!r}")
                specs.append(pack_item_groups(groups, caps, n_groups=len(index)))
            else:
                specs.append(pack_item_groups(groups, cap, n_groups=len(index)))
        device = self.model.engine.params.device
        return [spec.to(device) for spec in specs]

    def __call__(self, sequence: list, k: int = 1, allowed_items=None, diversity=None, candidate_pool=None, max_per_group=None,
                 return_probabilities: bool = False, min_probability=None, temperature: float = 1.0):
        """allowed_items: an iterable of items; only those are recommended.  diversity / candidate_pool / max_per_group /
        return_probabilities / min_probability / temperature: as in recommend_batch.  A call with any of them goes through
        recommend_batch."""
        calibrated = return_probabilities or min_probability is not None or not (isinstance(temperature, numbers.Real) and temperature == 1.0)
        if allowed_items is not None or diversity is not None or candidate_pool is not None or max_per_group is not None or calibrated:
            return self.recommend_batch([sequence], k, allowed_items=allowed_items, diversity=diversity, candidate_pool=candidate_pool,
                                        max_per_group=max_per_group, return_probabilities=return_probabilities,
                                        min_probability=min_probability, temperature=temperature)[0]
        tokenizer = self.dataloader.get_tokenizer()
        batch = self.dataloader.prepare_inference(list(sequence))
        batch = {key: torch.from_numpy(np.asarray(v)) for key, v in batch.items()}
        blocked = set(tokenizer.tokenize(list(sequence))) | {0, 1, 2}
        ranking, _, _, _ = self.model.rank_items_tensor(batch, None)      # [1, V]: the whole vocabulary, best first
        # the best k ids outside `blocked` are among the first k + |blocked| entries
        head = ranking[0, :k + len(blocked)].cpu().tolist()
        top = [i for i in head if i not in blocked][:k]
        items = tokenizer.detokenize(top)
        return items[0] if k == 1 else items

    def recommend_batch(self, sequences, k: int = 1, allowed_items=None, allowed_items_per_user=None, diversity=None,
                        candidate_pool=None, max_per_group=None, return_probabilities: bool = False, min_probability=None,
                        temperature: float = 1.0, sample_seed=None, user_streams=None, calibrate_by=None, calibrate_to: str = "history",
                        calibration=None) -> list:
        """Recommender(...)(seq, k) for every sequence of `sequences`, from one batched forward and one full-catalogue top-k.
        allowed_items: one iterable of items (detokenized values) for all users; allowed_items_per_user: one iterable per sequence
        (identical lists share one filter).  Only allowed items are recommended; items the vocabulary does not know are ignored.
        With k = 1 a user for whom nothing is left to recommend gets None, with or without a filter (every item seen or excluded).
        diversity: None or 0 = the k best items, as before; a number up to 1 = the k items are picked from the candidate_pool best
        (default min(1024, max(10 k, 50))) by greedy Maximal Marginal Relevance, so that they are less alike (recommend_tensor).
        max_per_group: (labels, cap) or a list of at most 4 such pairs -- at most cap of the k items share a group.  labels maps an
        item to a hashable group label (a mapping or a callable; unknown or absent items are in no group), cap is an int or a mapping
        label -> int.  The k items are picked from the candidate_pool best under the caps (b4r_rerank_quota); a user whose pool holds
        fewer than k admissible items gets a shorter list: a larger candidate_pool is the remedy.
        return_probabilities: every entry is an (item, probability) pair instead of an item: the softmax of the scores / temperature
        over the items the user could have been served (the seen items and the filter applied), for the items actually returned.
        min_probability: a number in [0, 1]; entries with a smaller probability are dropped (the rest keep their order), and a k = 1
        user left with nothing gets None.  temperature (finite, > 0) needs one of the two, or sample_seed.  Still one read-back of
        the lists per call.
        sample_seed: None = the k best items; an integer in [0, 2^64) = the k items are DRAWN without replacement from the softmax of
        the scores / temperature over the items the user could be served (b4r_sample_full), or over the candidate_pool best of them
        when candidate_pool is given (b4r_sample_pool), and returned in draw order: exploration traffic, propensity-logged lists.
        user_streams: one integer per sequence (a user id, a request counter): the user's noise stream, so that a user draws the
        same list under the same seed whatever batch they ride in (None: the position in the batch).  return_probabilities gives the
        probability of each drawn item over everything the user could be served (also when candidate_pool truncates the draw).  It
        does not combine with diversity or max_per_group.
        calibrate_by: None, or the items' categories as category_affinity takes them (a mapping or a callable from an item to its
        label, or one integer label per token id [V]; at most 1024 categories) -- the k items are picked from the candidate_pool best
        so that the list's category mix follows the user's own (b4r_rerank_calibrated: a user with 70 % drama and 30 % comedy gets
        about 7 and 3 of 10, not 10 dramas).  calibrate_to: "history" = the category counts of the user's sequence inside the model's
        window, "affinity" = the user's probability of picking from each category next (category_affinity's).  calibration: the
        weight of the category mix against the relevance, a number in [0, 1] (default 0.5; 0 = the k best items).  It does not
        combine with diversity, max_per_group or sample_seed."""
        sequences = [list(seq) for seq in sequences]
        serve = self._recommend_options(len(sequences), k, allowed_items, allowed_items_per_user, diversity, candidate_pool, max_per_group,
                                        return_probabilities, min_probability, temperature, sample_seed, user_streams, calibrate_by,
                                        calibrate_to, calibration)
        if not sequences:
            return []
        batch, exclude = self._requests(sequences)
        return self._recommend_requests(batch, exclude, len(sequences), serve)

    def _recommend_options(self, n: int, k, allowed_items, allowed_items_per_user, diversity, candidate_pool, max_per_group,
                           return_probabilities, min_probability, temperature, sample_seed, user_streams, calibrate_by, calibrate_to,
                           calibration) -> dict:
        """recommend_batch's keywords for n users, checked and made ready for the model (the filters, the quota specs and the labels
        are packed once per call): what _recommend_requests takes."""
        calibrated = bool(return_probabilities) or min_probability is not None
        sampled = sample_seed is not None
        if calibrate_by is None:
            if calibration is not None:
                raise ValueError("calibration is the weight of the calibrated re-ranking: give calibrate_by as well")
        else:
            if diversity is not None or max_per_group is not None or sampled:
                raise ValueError("calibrate_by does not combine with diversity, max_per_group or sample_seed")
            if calibrate_to not in engine_mod.CALIBRATION_TARGETS:
                raise ValueError(f"calibrate_to is one of {list(engine_mod.CALIBRATION_TARGETS)}, got {calibrate_to!r}")
            engine_mod.check_calibration_args(k, candidate_pool, 0.5 if calibration is None else calibration)
        if sampled:
            sample_seed = engine_mod.check_sample_seed(sample_seed)
            if diversity is not None or max_per_group is not None:
                raise ValueError("sample_seed does not combine with diversity or max_per_group")
        if user_streams is not None:
            if not sampled:
                raise ValueError("user_streams are the noise streams of a sampled call: give sample_seed as well")
            user_streams = engine_mod.check_sample_streams(user_streams)
        if min_probability is not None:
            if isinstance(min_probability, bool) or not isinstance(min_probability, numbers.Real) or not 0.0 <= min_probability <= 1.0:
                raise ValueError(f"min_probability must be a number in [0, 1], got {min_probability!r}")
        if not calibrated and not sampled and not (isinstance(temperature, numbers.Real) and temperature == 1.0):
            raise ValueError("temperature scales the probabilities: give return_probabilities, min_probability or sample_seed as well")
        allow, user_filter = self._allow_filters(n, allowed_items, allowed_items_per_user)
        quotas = None if max_per_group is None else self._item_groups(max_per_group)   # packed once per call
        calibrate = None
        if calibrate_by is not None:
            labels, G, _ = self._affinity_labels(calibrate_by)
            calibrate = (labels, G, calibrate_to)
        return dict(k=k, allow=allow, user_filter=user_filter, user_streams=user_streams, min_probability=min_probability,
                    return_probabilities=return_probabilities,
                    model=dict(diversity=diversity, pool=candidate_pool, max_per_group=quotas, return_distribution=calibrated,
                               temperature=temperature, sample_seed=sample_seed, calibrate=calibrate,
                               calibration=None if calibrate is None else (0.5 if calibration is None else calibration)))

    def _recommend_requests(self, batch, exclude, n: int, serve: dict) -> list:
        """The n users' lists from their requests (batch, exclude: _requests' pair, on the host or on the device) under the options
        `serve` (_recommend_options): one recommend_tensor call, one read-back of the lists, the ids back to items."""
        k, user_filter, user_streams = serve["k"], serve["user_filter"], serve["user_streams"]
        min_probability, return_probabilities = serve["min_probability"], serve["return_probabilities"]
        calibrated = serve["model"]["return_distribution"]
        tokenizer = self.dataloader.get_tokenizer()
        # one filter index and one stream per ranked slot: the slots of recommend_tensor are those with masked_lm_weights != 0, in
        # batch order
        row_filter = slot_streams = None
        if user_streams is not None and user_streams.numel() != n:
            raise ValueError(f"{user_streams.numel()} user streams for {n} sequences")
        if user_filter is not None or user_streams is not None:
            slot_user = torch.nonzero(batch["masked_lm_weights"] != 0, as_tuple=True)[0].cpu()
            row_filter = None if user_filter is None else user_filter[slot_user]
            slot_streams = None if user_streams is None else user_streams[slot_user]
        got = self.model.recommend_tensor(batch, k=k, exclude_seen=False, exclude=exclude, allow=serve["allow"], row_filter=row_filter,
                                          sample_streams=slot_streams, **serve["model"])
        ids, slots = got[0], got[2]
        P = int(batch["masked_lm_positions"].shape[1])
        first = {}
        for i, s in enumerate(slots.cpu().tolist()):   # __call__ ranks the first weighted slot of its one-row batch
            first.setdefault(s // P, i)
        prob_h = None
        if calibrated:
            # ids and probabilities in one copy: an id is exact in float64
            both = torch.cat([ids.to(torch.float64), torch.exp(got[3]["logp"].to(torch.float64))], dim=1).cpu()
            ids_h, prob_h = both[:, :ids.shape[1]].to(torch.int64).tolist(), both[:, ids.shape[1]:].tolist()
        else:
            ids_h = ids.cpu().tolist()
        least = 0.0 if min_probability is None else float(min_probability)
        out = []
        for b in range(n):
            top = [i for i in ids_h[first[b]] if i >= 0] if b in first else []
            if prob_h is not None:
                kept = [(i, p) for i, p in zip(ids_h[first[b]], prob_h[first[b]]) if i >= 0 and p >= least] if b in first else []
                top = [i for i, _ in kept]
            items = tokenizer.detokenize(top)
            if return_probabilities:
                items = [(item, p) for item, (_, p) in zip(items, kept)]
            out.append((items[0] if items else None) if k == 1 else items)   # None: nothing is left to recommend (filtered or not)
        return out

    def allocate(self, sequences, stock, k: int = 10, candidate_pool=None, allowed_items=None, user_ids=None,
                 return_probabilities: bool = True):
        """recommend_batch when some items are limited: `stock` maps each limited item to the units on offer (500 coupons, a listing
        that exists once, the seats of an event, "this campaign reaches at most c users"); an item it does not name is unlimited, an
        item the vocabulary does not know is ignored.  Every user gets at most k items and no item is handed out more often than its
        stock, over all users of the call: a contended item goes to the users most likely to take it, and a user who loses it gets
        the next item of their own candidate_pool best (default min(1024, max(10 k, 50))) instead -- a user whose pool yields fewer
        than k under the stock gets a shorter list, and a larger candidate_pool is the remedy.  The utilities are the items'
        probabilities under each user's catalogue softmax (the seen items and allowed_items applied), which is what makes different
        users comparable; ties go to the lower entry of user_ids (one integer per sequence; None: the position in the batch).
        Returns (lists, remaining): one list per user of (item, probability) pairs -- of items with return_probabilities=False --
        in the user's own order of preference, and {item: units left} for the items of `stock` the vocabulary knows.  Passing
        `remaining` as the stock of the next call serves the stock first come, first served: the result then depends on how the users
        are cut into calls.  One batched call (model.allocate_tensor); the pools are never read back, only the lists are."""
        sequences = [list(seq) for seq in sequences]
        serve = self._allocate_options(len(sequences), stock, k, candidate_pool, allowed_items, user_ids, return_probabilities)
        if not sequences:
            return [], dict(serve["left"])
        batch, exclude = self._requests(sequences)
        return self._allocate_requests(batch, exclude, len(sequences), serve)

    def _allocate_options(self, n: int, stock, k, candidate_pool, allowed_items, user_ids, return_probabilities) -> dict:
        """allocate's keywords for n users, checked and made ready for the model: what _allocate_requests takes.  left: the stock
        of the known items as given, which is what remains when there is nobody to serve."""
        if not hasattr(stock, "items"):
            raise ValueError("stock maps each limited item to its units: a mapping")
        k, pool, _ = engine_mod.check_rerank_args(k, candidate_pool, 0.0)
        engine_mod.check_allocate_args(k, n, pool)
        uid = engine_mod.check_allocate_user_ids(user_ids, n)
        names = list(stock)
        tokens = self._token_ids(names).tolist()
        by_token = {}
        for name, t in zip(names, tokens):
            if t >= 0:
                by_token[t] = stock[name]
        capacity = engine_mod.stock_capacity(by_token, self.model.vocab_size)
        known = [(name, t) for name, t in zip(names, tokens) if t >= 0]
        left = {name: int(capacity[t]) for name, t in known}
        allow, _ = self._allow_filters(n, allowed_items, None)
        return dict(k=k, pool=pool, capacity=capacity, allow=allow, user_ids=uid, known=known, left=left,
                    return_probabilities=bool(return_probabilities))

    def _allocate_requests(self, batch, exclude, n: int, serve: dict):
        """The n users' lists and the remaining stock from their requests (batch, exclude: _requests' pair, on the host or on the
        device): one allocate_tensor call, one read-back of the lists and of the stock."""
        k = serve["k"]
        slot_uid = None
        if serve["user_ids"] is not None:           # one id per ranked slot, as in _recommend_requests
            slot_uid = serve["user_ids"][torch.nonzero(batch["masked_lm_weights"] != 0, as_tuple=True)[0].cpu()]
        ids, util, slots, info = self.model.allocate_tensor(batch, serve["capacity"], k=k, pool=serve["pool"], calibrated=True, user_ids=slot_uid,
                                                            exclude_seen=False, exclude=exclude, allow=serve["allow"])
        P = int(batch["masked_lm_positions"].shape[1])
        first = {}
        for i, s in enumerate(slots.cpu().tolist()):
            first.setdefault(s // P, i)
        # ids, probabilities and the stock in one copy: an id and a count are exact in float64
        both = torch.cat([ids.to(torch.float64).reshape(-1), torch.exp(util.to(torch.float64)).reshape(-1),
                          info["remaining"].to(torch.float64)]).cpu()
        nk = ids.numel()
        ids_h = both[:nk].to(torch.int64).reshape(ids.shape).tolist()
        prob_h = both[nk:2 * nk].reshape(ids.shape).tolist()
        rem_h = both[2 * nk:].to(torch.int64).tolist()
        tokenizer = self.dataloader.get_tokenizer()
        out = []
        for b in range(n):
            kept = [(i, p) for i, p in zip(ids_h[first[b]], prob_h[first[b]]) if i >= 0] if b in first else []
            items = tokenizer.detokenize([i for i, _ in kept])
            out.append([(item, p) for item, (_, p) in zip(items, kept)] if serve["return_probabilities"] else items)
        return out, {name: rem_h[t] for name, t in serve["known"]}

    def open_sessions(self, max_users: int, history_capacity=None):
        """A SessionStore (apps/session_store.py) for max_users users: their histories stay on the device, `append` adds events and
        `recommend(user_keys)` serves recommend_batch's lists without preparing the histories on the host.  history_capacity: the
        items kept per user (default max(max_seq_len - 1, 256); below max_seq_len - 1 raises ValueError) -- a user's exclusions are
        their last history_capacity items, the full history as long as it is no longer than that."""
        from .session_store import SessionStore
        return SessionStore(self, max_users, history_capacity)

    def item_ranks(self, sequences, items=None, items_per_user=None, allowed_items=None, allowed_items_per_user=None) -> list:
        """Where given items stand for every user: "X is at 312 of 26 000 for this user" -- the position the item has in
        recommend_batch's order (the same exclusions: every item of the user's sequence; the same filters), from one batched forward,
        one b4r_item_ranks sweep and one read-back, however many items are asked about.  items: one iterable of items for all users,
        or items_per_user: one iterable per sequence.  Returns per user a list with one dict per asked item, in the order given:
          item   the item as given
          rank   its 1-based position among the items the user could be served; None for an item the vocabulary does not know,
                 that the user has seen, or that the filter does not allow
          of     the number of items the user could be served
          score  the item's score (None for an item the vocabulary does not know)."""
        if (items is None) == (items_per_user is None):
            raise ValueError("give items or items_per_user, one of them")
        sequences = [list(seq) for seq in sequences]
        if items is not None:
            asked = [list(items)] * len(sequences)
        else:
            asked = [list(it) for it in items_per_user]
            if len(asked) != len(sequences):
                raise ValueError(f"{len(asked)} item lists for {len(sequences)} sequences")
        allow, user_filter = self._allow_filters(len(sequences), allowed_items, allowed_items_per_user)
        if not sequences:
            return []
        if items is not None:
            tokens = [self._token_ids(asked[0]).tolist()] * len(sequences)
        else:
            tokens = [self._token_ids(it).tolist() for it in asked]
        batch, exclude = self._requests(sequences)
        slot_user = torch.nonzero(batch["masked_lm_weights"] != 0, as_tuple=True)[0]
        row_filter = None if user_filter is None else user_filter[slot_user]
        query = self._padded_ids(tokens)[slot_user]
        got = self.model.item_ranks_tensor(batch, query, exclude_seen=False, exclude=exclude, allow=allow, row_filter=row_filter)
        Q = int(query.shape[1])
        # ranks, scores, n and the slots in one copy: an int32 and an fp32 are exact in float64
        both = torch.cat([got["ranks"].to(torch.float64), got["scores"].to(torch.float64), got["n"].to(torch.float64)[:, None],
                          got["slot_index"].to(torch.float64)[:, None]], dim=1).cpu()
        P = int(batch["masked_lm_positions"].shape[1])
        first = {}
        for i, s in enumerate(both[:, 2 * Q + 1].to(torch.int64).tolist()):   # the first weighted slot of the user's row, as recommend_batch
            first.setdefault(s // P, i)
        rows = both.tolist()
        out = []
        for b, its in enumerate(asked):
            if b not in first:
                out.append([{"item": item, "rank": None, "of": 0, "score": None} for item in its])
                continue
            row = rows[first[b]]
            n = int(row[2 * Q])
            out.append([{"item": item, "rank": int(row[j]) if row[j] > 0 else None, "of": n,
                         "score": row[Q + j] if tokens[b][j] >= 0 else None} for j, item in enumerate(its)])
        return out

    def recommend_sequences(self, sequences, steps: int, beams: int = 1, expand=None, allowed_items=None, allowed_items_per_user=None,
                            temperature: float = 1.0, sample_seed=None, user_streams=None, return_probabilities: bool = False) -> list:
        """The next `steps` items of every sequence IN ORDER, each one conditioned on the ones before (queue continuation, "watch
        these three next", simulated trajectories): one batched BERT4RecModel.recommend_sequence_tensor call -- the items are
        appended on the device between the forwards -- and one read-back.
        beams = 1: per user a list of `steps` items, shorter when nothing was left to recommend: the greedy path (every step's best
        item), or with sample_seed a path drawn step by step from the softmax of the scores / temperature (user_streams: one integer
        per sequence, the user's noise stream, so that a user rolls out the same path whatever batch they ride in).
        beams > 1: beam search with `expand` candidates per beam (default beams); per user a list of up to `beams` (items,
        log_probability) pairs, the most probable path first.
        allowed_items / allowed_items_per_user: as in recommend_batch, applied at every step.  An item is never recommended twice on
        a path, nor when it occurs anywhere in the user's sequence (also before the model's window).
        return_probabilities: every item becomes an (item, probability) pair, the probability among the items the user could be
        served at that step."""
        steps, beams, expand = engine_mod.check_rollout_args(steps, beams, expand, temperature, sample_seed, bool(return_probabilities))
        if user_streams is not None:
            if sample_seed is None:
                raise ValueError("user_streams are the noise streams of a sampled call: give sample_seed as well")
            user_streams = engine_mod.check_sample_streams(user_streams)
        tokenizer = self.dataloader.get_tokenizer()
        sequences = [list(seq) for seq in sequences]
        if user_streams is not None and user_streams.numel() != len(sequences):
            raise ValueError(f"{user_streams.numel()} user streams for {len(sequences)} sequences")
        allow, row_filter = self._allow_filters(len(sequences), allowed_items, allowed_items_per_user)
        if not sequences:
            return []
        batch, exclude = self._requests(sequences)
        want_logp = bool(return_probabilities) or beams > 1
        ids, step_logp, logp, _ = self.model.recommend_sequence_tensor(
            batch, steps, beams=beams, expand=expand, exclude_seen=False, exclude=exclude, allow=allow, row_filter=row_filter,
            temperature=temperature, sample_seed=sample_seed, sample_streams=user_streams, return_logp=want_logp)
        U = len(sequences)
        if want_logp:
            # ids, probabilities and path totals in one copy: an id is exact in float64
            both = torch.cat([ids.reshape(U, -1).to(torch.float64), torch.exp(step_logp.reshape(U, -1).to(torch.float64)),
                              logp.reshape(U, -1).to(torch.float64)], dim=1).cpu()
            n = beams * steps
            ids_h = both[:, :n].to(torch.int64).reshape(U, beams, steps).tolist()
            prob_h = both[:, n:2 * n].reshape(U, beams, steps).tolist()
            logp_h = both[:, 2 * n:].tolist()
        else:
            ids_h, prob_h, logp_h = ids.cpu().tolist(), None, None
        out = []
        for u in range(U):
            paths = []
            for b in range(beams):
                kept = [(i, None if prob_h is None else prob_h[u][b][t]) for t, i in enumerate(ids_h[u][b]) if i >= 0]
                items = tokenizer.detokenize([i for i, _ in kept])
                if return_probabilities:
                    items = [(item, p) for item, (_, p) in zip(items, kept)]
                if beams == 1:
                    paths = items
                elif kept:
                    paths.append((items, logp_h[u][b]))
            out.append(paths)
        return out

    def _group_labels(self, by_group):
        """by_group -> (labels int32 [V] with -1 = no group, the label each group index stands for).  A mapping (or a callable) from a
        detokenized item to a hashable label, as max_per_group takes it: an item it does not know, or maps to None, is in no group.
        Or one integer label per token id [V] (negative = no group), as pack_item_groups takes it: the labels come back as they are."""
        V = self.model.vocab_size
        look = by_group if callable(by_group) else getattr(by_group, "get", None)
        if look is None:
            groups = np.asarray(by_group)
            if groups.ndim != 1 or groups.shape[0] != V or groups.dtype.kind not in "iu":
                raise ValueError(f"by_group maps an item to its label (a mapping or a callable) or holds one integer label per token id [{V}]")
            groups = np.where(groups < 0, -1, groups).astype(np.int64)
            if groups.size and groups.max() >= 1 << 31:
                raise ValueError("by_group labels must fit in int32")
            return torch.from_numpy(groups.astype(np.int32)), None
        groups, index = self._label_tokens(look)
        return torch.from_numpy(groups.astype(np.int32)), list(index)

    def explain_batch(self, sequences, items=None, k: int = 1, top: int = 3, window=None, by_group=None, allowed_items=None,
                      allowed_items_per_user=None, temperature: float = 1.0) -> list:
        """Why each item is recommended ("because you watched X"), for every sequence of `sequences`: one history item at a time is
        removed, the model runs again, and the history items whose removal costs the recommended item the most log probability are
        its reasons (BERT4RecModel.explain_tensor: the occluded rows are built on the device; one batched call, one read-back).
        items: None = the user's own top k, which are recommend_batch's items under the same filters; else one list of items per
        sequence (an item the vocabulary does not know is explained by nothing).  top: the reasons per item; window: only the
        `window` most recent history items are tried (None: all the model sees); top <= window.
        by_group: explain by category instead of by item -- a mapping (or a callable) from an item to its label, or one integer label
        per token id [V]: all history items of one category are removed together.
        allowed_items / allowed_items_per_user / temperature: as in recommend_batch; the probabilities are over the items the user
        could be served.
        Returns per sequence a list of (item, probability, reasons), the explained items in the order given (an own item that does not
        exist, k beyond what is left, is dropped).  reasons = [(history_item, delta_logp), ...], or with by_group [(label, delta_logp,
        n_items_removed), ...]: best first; delta_logp > 0 says the recommendation leans on it, < 0 that it was held back by it."""
        engine_mod.check_temperature(temperature)
        engine_mod.check_explain_args(top, window, engine_mod.EXPLAIN_MAX_UNITS)   # (the model checks them against its own length)
        sequences = [list(seq) for seq in sequences]
        if items is None:
            k = engine_mod.check_rank_full_args(k)
            if k < 1:
                raise ValueError(f"k must lie in [1, {engine_mod.RANK_FULL_MAX_K}], got {k}")
        else:
            items = [list(row) for row in items]
            if len(items) != len(sequences):
                raise ValueError(f"{len(items)} item lists for {len(sequences)} sequences")
            if sequences and not 1 <= max(len(row) for row in items) <= engine_mod.RANK_FULL_MAX_K:
                raise ValueError(f"between 1 and {engine_mod.RANK_FULL_MAX_K} items are explained per sequence")
        allow, row_filter = self._allow_filters(len(sequences), allowed_items, allowed_items_per_user)
        labels = names = None
        if by_group is not None:
            labels, names = self._group_labels(by_group)
        if not sequences:
            return []
        tokenizer = self.dataloader.get_tokenizer()
        batch, exclude = self._requests(sequences)
        target = k if items is None else self._padded_ids([self._token_ids(row).tolist() for row in items])
        got = self.model.explain_tensor(batch, target, top=top, labels=labels, window=window, exclude_seen=False, exclude=exclude,
                                        allow=allow, row_filter=row_filter, temperature=temperature)
        U, K = (int(x) for x in got["target_ids"].shape)
        # everything in one copy: ids and counts are exact in float64
        unit = got["top_label"] if labels is not None else got["top_item"]
        removed = got["removed"].gather(1, got["top_w"].clamp(min=0).to(torch.int64).reshape(U, -1))
        both = torch.cat([got["target_ids"].to(torch.float64), torch.exp(got["base_logp"].to(torch.float64)),
                          unit.reshape(U, -1).to(torch.float64), got["top_delta"].reshape(U, -1).to(torch.float64),
                          removed.to(torch.float64), got["top_w"].reshape(U, -1).to(torch.float64)], dim=1).cpu()
        n = K * top
        ids_h = both[:, :K].to(torch.int64).tolist()
        prob_h = both[:, K:2 * K].tolist()
        unit_h, delta_h, removed_h, w_h = (both[:, 2 * K + s * n:2 * K + (s + 1) * n].reshape(U, K, top).tolist() for s in range(4))
        out = []
        for u in range(U):
            rows = []
            for i in range(K):
                given = items is not None and i < len(items[u])
                if ids_h[u][i] < 0 and not given:
                    continue                                       # nothing was left to recommend / the padding of a shorter list
                live = [t for t in range(top) if w_h[u][i][t] >= 0]
                if labels is not None:
                    reasons = [(int(unit_h[u][i][t]) if names is None else names[int(unit_h[u][i][t])], delta_h[u][i][t],
                                int(removed_h[u][i][t])) for t in live]
                else:
                    reasons = [(h, delta_h[u][i][t]) for h, t in zip(tokenizer.detokenize([int(unit_h[u][i][t]) for t in live]), live)]
                name = items[u][i] if given else tokenizer.detokenize([ids_h[u][i]])[0]
                rows.append((name, prob_h[u][i], reasons))
            out.append(rows)
        return out

    def explain(self, sequence: list, items=None, k: int = 1, top: int = 3, window=None, by_group=None, allowed_items=None,
                temperature: float = 1.0) -> list:
        """explain_batch for one sequence: a list of (item, probability, reasons)."""
        return self.explain_batch([sequence], None if items is None else [list(items)], k=k, top=top, window=window, by_group=by_group,
                                  allowed_items=allowed_items, temperature=temperature)[0]

    def audience(self, items, sequences, k: int = 100, min_probability=None, user_ids=None, batch_size: int = 256, allowed_items=None,
                 allowed_items_per_user=None, temperature: float = 1.0) -> list:
        """Given items, which users?  For every item of `items` (raw item keys) the k users most likely to take it next, out of the
        users whose histories are `sequences`: "notify the 10 000 users most likely to want this release", "how many users would
        take it with probability >= 1 %", "what demand to expect for these titles".  The users go through the model in batches of
        batch_size (BERT4RecModel.audience_tensor); the k best users of every item, its reach and its expected demand stay on the
        device while the batches go by and are read back once, after the last one.
        user_ids: the users' names, one per sequence (default 0 .. n-1).  A user who has the item anywhere in their sequence, or who
        may not be served it (allowed_items / allowed_items_per_user, as in recommend_batch), is never in its audience.
        min_probability: None, or a number in (0, 1]: reach counts the users with at least that probability.
        Returns one dict per item, in the order given: {"users": [(user, probability), ...] best first (ties to the user earlier in
        `sequences`), "reach": the users who could be served it (with min_probability: with at least that probability),
        "expected_demand": the sum of all those users' probabilities}.  An item the vocabulary does not know has no audience."""
        engine_mod.check_temperature(temperature)
        k, _ = engine_mod.check_audience_args(k, min_probability)
        batch_size = engine_mod._int_in(batch_size, 1, (1 << 31) - 1, "batch_size")
        items = list(items)
        sequences = [list(seq) for seq in sequences]
        names = list(range(len(sequences))) if user_ids is None else list(user_ids)
        if len(names) != len(sequences):
            raise ValueError(f"{len(names)} user ids for {len(sequences)} sequences")
        allow, user_filter = self._allow_filters(len(sequences), allowed_items, allowed_items_per_user)
        if not items:
            return []
        item_ids = self._token_ids(items)
        if allow is not None:
            allow = engine_mod.pack_item_filter(allow).to(self.model.engine.params.device)   # packed once, for every batch
        state = self.model.engine.audience_state(item_ids, k)
        for b0 in range(0, len(sequences), batch_size):
            batch, exclude = self._requests(sequences[b0:b0 + batch_size])
            row_filter = None if user_filter is None else user_filter[b0:b0 + batch_size]
            state = self.model.audience_tensor(batch, item_ids, state=state, k=k, user_ids=torch.arange(b0, b0 + len(exclude)),
                                               min_probability=min_probability, exclude_seen=False, exclude=exclude, allow=allow,
                                               row_filter=row_filter, temperature=temperature)
        # everything in one copy: the probabilities travel as the bits of their float64
        both = torch.cat([state["users"], torch.exp(state["logp"].to(torch.float64)).view(torch.int64), state["reach"][:, None],
                          state["demand"][:, None]], dim=1).cpu()
        users_h = both[:, :k].tolist()
        prob_h = both[:, k:2 * k].contiguous().view(torch.float64).tolist()
        reach_h, demand_h = both[:, 2 * k].tolist(), both[:, 2 * k + 1].tolist()
        return [{"users": [(names[u], p) for u, p in zip(users_h[j], prob_h[j]) if u >= 0], "reach": int(reach_h[j]),
                 "expected_demand": demand_h[j] / engine_mod.AUDIENCE_DEMAND_ONE} for j in range(len(items))]

    def _affinity_labels(self, by_group):
        """by_group (as _group_labels takes it) -> (labels int32 [V], the number of groups G, the name of each group or None)"""
        labels, names = self._group_labels(by_group)
        labels, G = engine_mod.check_item_group_labels(labels, self.model.vocab_size, None if names is None else (len(names) or None))
        return labels, G, names

    def category_affinity(self, sequences, by_group, top=None, allowed_items=None, temperature: float = 1.0) -> list:
        """P(next item is of category c | user) for every sequence: which shelf to show first, what share of a user's taste a genre
        holds (BERT4RecModel.group_affinity_tensor: one batched forward, two sweeps over the catalogue, no [users, V] probabilities,
        one read-back).  by_group: a mapping (or a callable) from an item to its label, or one integer label per token id [V], as
        explain_batch takes it.  The probabilities are over the items the user could be served: not the items of their own
        sequence, and with allowed_items only those.  Returns per sequence [(label, probability), ...], best first (ties in the order
        the labels first appear), the `top` best when given; a category the user can be served nothing of is left out.  The
        probabilities of one user sum to at most 1: the rest belongs to the items without a label."""
        engine_mod.check_temperature(temperature)
        if top is not None:
            top = engine_mod._int_in(top, 1, engine_mod.GROUP_MASS_MAX_G, "top")
        sequences = [list(seq) for seq in sequences]
        allow, _ = self._allow_filters(len(sequences), allowed_items, None)
        labels, G, names = self._affinity_labels(by_group)
        if not sequences:
            return []
        batch, exclude = self._requests(sequences)
        got = self.model.group_affinity_tensor(batch, labels, G, exclude_seen=False, exclude=exclude, allow=allow, temperature=temperature)
        both = torch.cat([got["group_mass"], got["group_n"].to(torch.int64), got["slot_index"][:, None]], dim=1).cpu()
        return self._affinity_lists(both[:, :G], both[:, G:2 * G], both[:, 2 * G], int(batch["masked_lm_positions"].shape[1]),
                                    len(sequences), names, top)

    @staticmethod
    def _affinity_lists(mass, n, slots, P: int, n_users: int, names, top) -> list:
        """category_affinity's lists from the host copies of group_mass / group_n [R, G] and slot_index [R]: a user's first ranked slot
        counts, groups with n = 0 are dropped, the order is mass descending with ties to the lower group index."""
        first = {}
        for i, s in enumerate(slots.tolist()):
            first.setdefault(s // P, i)
        out = []
        for b in range(n_users):
            if b not in first:
                out.append([])
                continue
            m, c = mass[first[b]].tolist(), n[first[b]].tolist()
            order = sorted((g for g in range(len(m)) if c[g] > 0), key=lambda g: (-m[g], g))
            out.append([(g if names is None else names[g], m[g] / engine_mod.GROUP_MASS_ONE) for g in order[:top]])
        return out

    def category_audience(self, by_group, sequences, k: int = 100, min_probability=None, user_ids=None, batch_size: int = 256,
                          allowed_items=None, allowed_items_per_user=None, temperature: float = 1.0) -> list:
        """Given categories, which users?  `audience` with the categories of by_group in place of single items: for every category
        the k users most likely to take one of its items next, its reach and its expected demand -- the users of a genre campaign.
        The users go through the model in batches of batch_size (BERT4RecModel.group_audience_tensor) and the result is read back
        once; it does not depend on batch_size.  by_group: as category_affinity takes it; the other arguments are `audience`'s.
        Returns one dict per category, in the order the labels first appear (or by integer label): {"label", "users": [(user,
        probability), ...] best first, "reach", "expected_demand"}."""
        engine_mod.check_temperature(temperature)
        k, _ = engine_mod.check_audience_args(k, min_probability)
        batch_size = engine_mod._int_in(batch_size, 1, (1 << 31) - 1, "batch_size")
        sequences = [list(seq) for seq in sequences]
        names = list(range(len(sequences))) if user_ids is None else list(user_ids)
        if len(names) != len(sequences):
            raise ValueError(f"{len(names)} user ids for {len(sequences)} sequences")
        allow, user_filter = self._allow_filters(len(sequences), allowed_items, allowed_items_per_user)
        labels, G, group_names = self._affinity_labels(by_group)
        if allow is not None:
            allow = engine_mod.pack_item_filter(allow).to(self.model.engine.params.device)   # packed once, for every batch
        state = None
        for b0 in range(0, len(sequences), batch_size):
            batch, exclude = self._requests(sequences[b0:b0 + batch_size])
            row_filter = None if user_filter is None else user_filter[b0:b0 + batch_size]
            state = self.model.group_audience_tensor(batch, labels, G, state=state, k=k, user_ids=torch.arange(b0, b0 + len(exclude)),
                                                     min_probability=min_probability, exclude_seen=False, exclude=exclude,
                                                     allow=allow, row_filter=row_filter, temperature=temperature)
        if state is None:
            return [{"label": g if group_names is None else group_names[g], "users": [], "reach": 0, "expected_demand": 0.0}
                    for g in range(G)]
        both = torch.cat([state["users"], torch.exp(state["logp"].to(torch.float64)).view(torch.int64), state["reach"][:, None],
                          state["demand"][:, None]], dim=1).cpu()
        users_h = both[:, :k].tolist()
        prob_h = both[:, k:2 * k].contiguous().view(torch.float64).tolist()
        reach_h, demand_h = both[:, 2 * k].tolist(), both[:, 2 * k + 1].tolist()
        return [{"label": g if group_names is None else group_names[g],
                 "users": [(names[u], p) for u, p in zip(users_h[g], prob_h[g]) if u >= 0], "reach": int(reach_h[g]),
                 "expected_demand": demand_h[g] / engine_mod.AUDIENCE_DEMAND_ONE} for g in range(G)]

    def recommend_shelves(self, sequences, by_group, shelves: int = 3, k: int = 10, allowed_items=None, temperature: float = 1.0) -> list:
        """A page per user: the `shelves` categories the user is most likely to pick from next, each with its k best items
        (BERT4RecModel.recommend_shelves_tensor: one batched forward, the categories' item filters built once, ONE full-catalogue
        top-k over the users x shelves rows, one read-back).  by_group: as category_affinity takes it, at most 1024 categories.
        Each shelf's items are what recommend_batch returns with that category as the allow-list.  Returns per sequence
        [(label, probability, [item, ...]), ...], best category first; a user with fewer categories to be served from gets fewer
        shelves."""
        engine_mod.check_temperature(temperature)
        sequences = [list(seq) for seq in sequences]
        allow, _ = self._allow_filters(len(sequences), allowed_items, None)
        labels, G, names = self._affinity_labels(by_group)
        shelves, k = engine_mod.check_shelf_args(shelves, k, G)
        if not sequences:
            return []
        tokenizer = self.dataloader.get_tokenizer()
        batch, exclude = self._requests(sequences)
        group, mass, ids, _, slots = self.model.recommend_shelves_tensor(batch, labels, G, shelves=shelves, k=k, exclude_seen=False,
                                                                         exclude=exclude, allow=allow, temperature=temperature)
        R = int(slots.numel())
        both = torch.cat([group, mass, ids.reshape(R, shelves * k), slots[:, None]], dim=1).cpu()   # everything in one copy
        group_h, mass_h = both[:, :shelves].tolist(), both[:, shelves:2 * shelves].tolist()
        ids_h = both[:, 2 * shelves:2 * shelves + shelves * k].reshape(R, shelves, k).tolist()
        P = int(batch["masked_lm_positions"].shape[1])
        first = {}
        for i, s in enumerate(both[:, -1].tolist()):
            first.setdefault(s // P, i)
        out = []
        for b in range(len(sequences)):
            page = []
            for s in range(shelves if b in first else 0):
                g = group_h[first[b]][s]
                if g < 0:
                    continue
                items = tokenizer.detokenize([i for i in ids_h[first[b]][s] if i >= 0])
                page.append((g if names is None else names[g], mass_h[first[b]][s] / engine_mod.GROUP_MASS_ONE, items))
            out.append(page)
        return out

    def recommend_together(self, parties, k: int = 10, strategy: str = "additive", weights=None, min_member_probability=None,
                           allowed_items=None, return_members: bool = False) -> list:
        """Several users deciding together (a household choosing a film, friends choosing a game, a shared playlist): one list of k
        items per PARTY.  parties: a list of parties, each a list of 1 to 16 item sequences (its members' histories).  One batched
        BERT4RecModel.recommend_joint_tensor call over all members and one read-back.
        An item is recommended to a party only when no member has it anywhere in their sequence (and allowed_items, one iterable of
        items for everybody, holds it).  strategy ranks the items by the members' log probabilities of taking them next:
        "additive" (their sum; weights: one list of numbers >= 0 per party, a member's say), "least_misery" (the least happy
        member's), "most_pleasure" (the happiest member's).  min_member_probability q in (0, 1]: the veto -- an item some member
        takes with probability below q is not recommended.
        Returns per party [(item, score), ...], best first, shorter when the party could be served fewer than k items; with
        return_members [(item, score, [p_member, ...]), ...]: the probability each member takes the item next, the one
        recommend_batch(return_probabilities=True) gives that user for that item."""
        parties = [[list(seq) for seq in party] for party in parties]
        for party in parties:
            if not 1 <= len(party) <= engine_mod.JOINT_MAX_MEMBERS:
                raise ValueError(f"a party has between 1 and {engine_mod.JOINT_MAX_MEMBERS} members, got {len(party)}")
        M = max((len(party) for party in parties), default=1)
        rows = torch.full((len(parties), M), -1, dtype=torch.int64)
        sequences = []
        for p, party in enumerate(parties):
            rows[p, :len(party)] = torch.arange(len(sequences), len(sequences) + len(party))
            sequences.extend(party)
        w = None
        if weights is not None:
            weights = [list(ws) for ws in weights]
            if len(weights) != len(parties) or any(len(ws) != len(party) for ws, party in zip(weights, parties)):
                raise ValueError("weights holds one number per member: a list per party, as long as the party")
            w = torch.zeros((len(parties), M), dtype=torch.float32)
            for p, ws in enumerate(weights):
                w[p, :len(ws)] = torch.as_tensor(ws, dtype=torch.float32)
        engine_mod.check_joint_args(rows, k, strategy, w, min_member_probability, True, 1.0, len(sequences))
        allow, _ = self._allow_filters(len(sequences), allowed_items, None)
        if not parties:
            return []
        tokenizer = self.dataloader.get_tokenizer()
        batch, exclude = self._requests(sequences)
        got = self.model.recommend_joint_tensor(batch, rows, k=k, strategy=strategy, weights=w, min_member_probability=min_member_probability,
                                                exclude_seen=False, exclude=exclude, allow=allow, return_members=return_members)
        ids, scores = got[0], got[1]
        # everything in one copy: an id is exact in float64
        cols = [ids.to(torch.float64), scores.to(torch.float64)]
        if return_members:
            cols.append(torch.exp(got[3].to(torch.float64)).reshape(len(parties), -1))
        both = torch.cat(cols, dim=1).cpu()
        K = int(ids.shape[1])
        ids_h, scores_h = both[:, :K].to(torch.int64).tolist(), both[:, K:2 * K].tolist()
        prob_h = both[:, 2 * K:].reshape(len(parties), K, M).tolist() if return_members else None
        out = []
        for p, party in enumerate(parties):
            kept = [i for i, t in enumerate(ids_h[p]) if t >= 0]
            items = tokenizer.detokenize([ids_h[p][i] for i in kept])
            if return_members:
                out.append([(item, scores_h[p][i], prob_h[p][i][:len(party)]) for item, i in zip(items, kept)])
            else:
                out.append([(item, scores_h[p][i]) for item, i in zip(items, kept)])
        return out

    def similar_items(self, items, k: int = 10, metric: str = "cosine", allowed_items=None) -> list:
        """For every item of `items` the k nearest items of the learned item table, as detokenized lists (best first); metric
        "cosine" or "dot".  An item the vocabulary does not know gets an empty list.  allowed_items: only those are returned."""
        tokenizer = self.dataloader.get_tokenizer()
        items = list(items)
        if not items:
            return []
        allow = None if allowed_items is None else self._item_mask(allowed_items)
        ids, _ = self.model.similar_items_tensor(self._token_ids(items), k=k, metric=metric, allow=allow)
        return [tokenizer.detokenize([i for i in row if i >= 0]) for row in ids.cpu().tolist()]

    def list_quality(self, lists, item_counts=None) -> dict:
        """What recommendation lists are like beyond accuracy.  lists: an iterable of item lists (detokenized values, as __call__ and
        recommend_batch return them with k > 1; items the vocabulary does not know are ignored; at most 1024 items each).
        item_counts: how often each item was interacted with -- a mapping item -> count, or one count per token id [V].  Returns floats:
          ild       intra-list diversity: the mean over the lists with at least 2 items of the mean 1 - cosine (in the item table)
                    over the list's item pairs; 0.0 when no list has 2 items
          coverage  the distinct items in the lists over the catalogue size V - 3 (the vocabulary without [PAD] / [MASK] / [UNK])
          novelty   (with item_counts) the mean over the non-empty lists of the mean self-information -log2(count / all counts) of the
                    list's items
        One b4r_list_metrics call on the device; the sums are read back once."""
        V = self.model.vocab_size
        tokens = [self._known_tokens(list(lst)) for lst in lists]
        out = {"ild": 0.0, "coverage": 0.0}
        weight = None
        if item_counts is not None:
            if hasattr(item_counts, "items"):
                counts = np.zeros(V, dtype=np.float64)
                for item, c in item_counts.items():
                    for t in self._known_tokens([item]):
                        counts[t] += float(c)
            else:
                counts = np.asarray(item_counts, dtype=np.float64).reshape(-1)
                if counts.shape[0] != V:
                    raise ValueError(f"item_counts holds {counts.shape[0]} counts for a vocabulary of {V}")
            weight = torch.from_numpy(item_self_information(counts))
            out["novelty"] = 0.0
        if not any(tokens):
            return out
        ids = self._padded_ids(tokens)
        engine = self.model.engine
        dev = engine.params.device
        exposure = torch.zeros(V, dtype=torch.int64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        counts_d = torch.zeros(2, dtype=torch.int64, device=dev)
        engine.list_metrics(ids, None, weight, exposure=exposure, sums=sums, counts=counts_d)
        back = torch.cat([sums, counts_d.to(torch.float64), (exposure[SPECIAL_IDS:] > 0).sum().to(torch.float64).reshape(1)]).cpu().tolist()
        if back[2] > 0:
            out["ild"] = back[0] / back[2]
        if weight is not None and back[3] > 0:
            out["novelty"] = back[1] / back[3]
        out["coverage"] = back[4] / max(V - SPECIAL_IDS, 1)
        return out
