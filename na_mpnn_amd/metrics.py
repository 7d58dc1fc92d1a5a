"""Training / validation metrics of the reference's loop (na_metric_manager.py; na_model_utils.py:148-166; na_run.py:240-326).

``MetricManager`` / ``generate_metric_manager`` are drop-ins for ``na_metric_manager``: the same modes, row and column names, table,
normalisation and print string.  On HIP tensors a batch is reduced into a device fp64 table by ``namp_train_metrics`` (two launches,
csrc/namp_metrics.h) with no host synchronisation: the table reaches the host once, when ``metrics`` is read (``compute_metrics``,
``create_print_string``).  ``accumulate_from_log_probs`` is the fused form of the reference's epilogue — argmax, accuracy, the
canonical-pair accuracy and the per-token label-smoothed loss come from ``log_probs`` inside the same launch.  Host tensors take a
stock-op restatement.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import hip, spec

_QUANTITIES = ["weights", "canonicalBasePairWeights", "loss", "accuracy", "canonicalBasePairAccuracy"]   # kernel order, then true / pred counts


def _pairs(pdb_dataset):
    pairs = getattr(pdb_dataset, "na_canonical_base_pair_ints", pdb_dataset)
    return [(int(a), int(b)) for a, b in pairs]


def _pair_bits(pairs, V):
    bits = (C.c_ulonglong * 64)()
    for a, b in pairs:
        if 0 <= a < V and 0 <= b < V:
            bits[a] |= 1 << b
    return bits


def _ref(t, keep):
    """NampTensorRef of a [B, L] tensor (made contiguous; the temporary is kept alive in ``keep`` until the launch is enqueued)."""
    if t is None:
        return hip.NampTensorRef(None, 0, 0)
    if not t.is_contiguous():
        t = t.contiguous()
    name = str(t.dtype).replace("torch.", "")
    if name not in hip.NAMP_DT:
        t, name = t.double(), "float64"
    keep.append(t)
    return hip.NampTensorRef(t.data_ptr(), hip.NAMP_DT[name], 0)


def _batch(S, cbp_mask, cbp_index, V, keep, log_probs=None):
    B, L = S.shape[0], S.shape[-1]
    m = hip.NampMetricBatch()
    m.G, m.L, m.V = S.numel(), L, V
    if log_probs is not None:
        lp = log_probs.contiguous().float()
        keep.append(lp)
        m.log_probs = lp.data_ptr()
    m.S, m.cbp_mask, m.cbp_index = _ref(S, keep), _ref(cbp_mask, keep), _ref(cbp_index, keep)
    return m


def _host_pair_accuracy(S_pred, cbp_mask, cbp_index, pairs):
    """Stock-op canonical-pair accuracy: the partner's prediction, then "is (own, partner) one of the pairs", times the mask."""
    partner = torch.gather(S_pred, 1, cbp_index)
    hit = torch.zeros_like(S_pred, dtype=torch.bool)
    for a, b in pairs:
        hit = hit | ((S_pred == a) & (partner == b))
    return hit.long() * cbp_mask


def compute_canonical_base_pair_accuracy(log_probs, canonical_base_pair_mask, canonical_base_pair_index, pdb_dataset):
    """[B, L] int64: 1 where the predicted residue and the prediction at ``canonical_base_pair_index`` form a canonical pair, times
    ``canonical_base_pair_mask`` (na_model_utils.py:148-166).  ``pdb_dataset``: anything with ``.na_canonical_base_pair_ints``, or
    the list of (int, int) pairs itself.  On a HIP device: one launch; an index outside [0, L) gives 0 there (the host path raises)."""
    pairs = _pairs(pdb_dataset)
    if not log_probs.is_cuda:
        return _host_pair_accuracy(torch.argmax(log_probs, -1), canonical_base_pair_mask, canonical_base_pair_index, pairs)
    V = log_probs.shape[-1]
    keep = []
    S_dummy = canonical_base_pair_index                  # S is not read in this mode; any [B, L] tensor of the right shape serves
    m = _batch(S_dummy, canonical_base_pair_mask, canonical_base_pair_index, V, keep, log_probs)
    m.pair_bits = _pair_bits(pairs, V)
    out = torch.empty(log_probs.shape[:-1], dtype=torch.int64, device=log_probs.device)
    hip.check(hip.lib().namp_canonical_pair_accuracy(C.byref(m), out.data_ptr(), None, hip.current_stream()), "canonical_pair_accuracy")
    return out


class MetricManager(object):
    """na_metric_manager.MetricManager with the table on the device while HIP batches are accumulated."""

    def __init__(self, restype_to_int, weight_metrics, sum_metrics, count_metrics, extra_metrics, dataset_names, polymer_mask_names,
                 interface_mask_names, canonical_base_pair_ints=None):
        self.restype_to_int = restype_to_int
        self.weight_metrics = weight_metrics
        self.sum_metrics = sum_metrics
        self.count_metrics = count_metrics
        self.extra_metrics = extra_metrics
        self.dataset_names = dataset_names
        self.polymer_mask_names = polymer_mask_names
        self.interface_mask_names = interface_mask_names
        if len(count_metrics) > hip.NAMP_METRIC_MAX_RES:
            raise ValueError(f"at most {hip.NAMP_METRIC_MAX_RES} count metrics")
        self.na_canonical_base_pair_ints = (spec.na_canonical_base_pair_ints(restype_to_int) if canonical_base_pair_ints is None
                                            else _pairs(canonical_base_pair_ints))

        self.all_mask_names = self.get_all_masks()
        self.mask_to_row = dict(zip(self.all_mask_names, range(len(self.all_mask_names))))
        self.row_to_mask = dict(zip(range(len(self.all_mask_names)), self.all_mask_names))
        self.metric_names = (list(weight_metrics) + list(sum_metrics) + ["pred" + r for r in count_metrics] + ["true" + r for r in count_metrics]
                             + list(extra_metrics))
        self.metric_to_col = dict(zip(self.metric_names, range(len(self.metric_names))))

        # the kernel's quantity q lands in column _col_of[q] (-1: not a metric of this manager; e.g. the "all" mode's sum metric
        # "canonialBasePairAccuracy" is spelt so that the reference never fills it, and neither do we)
        present = {"weights": "weights" in weight_metrics, "canonicalBasePairWeights": "canonicalBasePairWeights" in weight_metrics,
                   "loss": "loss" in sum_metrics, "accuracy": "accuracy" in sum_metrics,
                   "canonicalBasePairAccuracy": "canonicalBasePairAccuracy" in sum_metrics}
        self._col_of = [self.metric_to_col[q] if present[q] else -1 for q in _QUANTITIES]
        self._col_of += [self.metric_to_col["true" + r] for r in count_metrics] + [self.metric_to_col["pred" + r] for r in count_metrics]
        self._res = [int(restype_to_int[r]) for r in count_metrics]
        self._ws = None
        self.zero_metrics()

    def get_all_masks(self):
        names = []
        for dataset_name in self.dataset_names:
            for polymer in [""] + list(self.polymer_mask_names):
                for interface in [""] + list(self.interface_mask_names):
                    names.append(dataset_name + ("_" + polymer if polymer else "") + ("_" + interface if interface else ""))
        return names

    # ---- the table: a host array, or a device tensor while HIP batches are being added ----
    @property
    def metrics(self):
        """The fp64 table [rows, columns] as a numpy array.  If HIP batches were accumulated, this read copies it to the host (one
        synchronising copy); the host array is then the table until the next HIP batch."""
        if self._dev is not None:
            self._host = self._dev.cpu().numpy()
            self._dev = None
        return self._host

    @metrics.setter
    def metrics(self, value):
        self._host = np.asarray(value, dtype=np.float64)
        self._dev = None

    def zero_metrics(self):
        self._host = np.zeros((len(self.mask_to_row), len(self.metric_to_col)), dtype=np.float64)
        self._dev = None
        self._err = None
        self._host_err = False

    def _device_table(self, device):
        if self._dev is None:
            if self._host.any():      # host rows from earlier batches: upload them without a blocking copy
                self._dev = torch.from_numpy(self._host).pin_memory().to(device, non_blocking=True)
            else:
                self._dev = torch.zeros(self._host.shape, dtype=torch.float64, device=device)
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=device)
        return self._dev

    def _rows(self, train_or_valid, polymer_masks, interface_masks):
        rows = []
        for polymer in [""] + list(polymer_masks):
            for interface in [""] + list(interface_masks):
                rows.append(self.mask_to_row[train_or_valid + ("_" + polymer if polymer else "") + ("_" + interface if interface else "")])
        return rows

    def _launch(self, m, keep, train_or_valid, mask_for_loss, polymer_masks, interface_masks, device):
        if len(polymer_masks) > 3 or len(interface_masks) > 2:
            raise ValueError("at most 3 polymer masks and 2 interface masks per batch")
        rows = self._rows(train_or_valid, polymer_masks, interface_masks)
        m.mask_for_loss = _ref(mask_for_loss, keep)
        m.n_polymer, m.n_interface = len(polymer_masks), len(interface_masks)
        for k, t in enumerate(polymer_masks.values()):
            m.row_polymer[k] = _ref(t, keep)
        for k, t in enumerate(interface_masks.values()):
            m.row_interface[k] = _ref(t, keep)
        m.n_res = len(self._res)
        for k, r in enumerate(self._res):
            m.res[k] = r
        table = self._device_table(device)
        need = hip.lib().namp_train_metrics_workspace(m.G, len(rows), m.n_res)
        if self._ws is None or self._ws.numel() < need or self._ws.device != table.device:
            self._ws = torch.empty(need, dtype=torch.float64, device=device)
        row_of = (C.c_int32 * len(rows))(*rows)
        col_of = (C.c_int32 * len(self._col_of))(*self._col_of)
        hip.check(hip.lib().namp_train_metrics(C.byref(m), table.data_ptr(), table.shape[1], row_of, col_of, self._ws.data_ptr(),
                                               self._err.data_ptr(), hip.current_stream()), "train_metrics")

    def accumulate(self, loss, accuracy, canonical_base_pair_accuracy, canonical_base_pair_mask, S_true, S_pred, train_or_valid,
                   mask_for_loss, polymer_masks, interface_masks):
        """na_metric_manager.MetricManager.accumulate: per-token loss / accuracy / canonical-pair accuracy given, masked sums added to
        the rows of ``train_or_valid``.  HIP tensors: two launches, no host synchronisation."""
        if not loss.is_cuda:
            return self._accumulate_host(loss, accuracy, canonical_base_pair_accuracy, canonical_base_pair_mask, S_true, S_pred,
                                         train_or_valid, mask_for_loss, polymer_masks, interface_masks)
        keep = []
        m = _batch(S_true, canonical_base_pair_mask, None, 1, keep)
        m.loss, m.accuracy = _ref(loss, keep), _ref(accuracy, keep)
        m.cbp_accuracy, m.S_pred = _ref(canonical_base_pair_accuracy, keep), _ref(S_pred, keep)
        self._launch(m, keep, train_or_valid, mask_for_loss, polymer_masks, interface_masks, loss.device)

    def accumulate_from_log_probs(self, log_probs, feature_dict, train_or_valid, mask_for_loss, polymer_masks, interface_masks, *,
                                  polymer_restype_masks, polymer_restype_nums, weight=0.1):
        """The reference's whole epilogue (loss_nll's accuracy, compute_canonical_base_pair_accuracy, argmax, loss_smoothed's per-token
        loss, accumulate; na_run.py:240-273) from ``log_probs``.  ``feature_dict`` supplies S, the protein / dna / rna masks of the
        loss, ``ppm_mask`` / ``aligned_ppm`` and ``canonical_base_pair_mask`` / ``_index`` (absent: all zero).  HIP tensors: two
        launches, no host synchronisation."""
        fd = feature_dict
        S = fd["S"]
        zeros = None
        cbp_mask, cbp_index = fd.get("canonical_base_pair_mask"), fd.get("canonical_base_pair_index")
        if cbp_mask is None or cbp_index is None:
            zeros = torch.zeros(S.shape, dtype=torch.int64, device=S.device)
            cbp_mask = zeros if cbp_mask is None else cbp_mask
            cbp_index = zeros if cbp_index is None else cbp_index
        loss_masks = {k: fd[k + "_mask"] if k + "_mask" in fd else polymer_masks[k] for k in ("protein", "dna", "rna")}
        ppm_mask, aligned_ppm = fd.get("ppm_mask"), fd.get("aligned_ppm")
        if not log_probs.is_cuda:
            from . import train
            S_pred = torch.argmax(log_probs, -1)
            accuracy = (S == S_pred).float()
            bad = (cbp_index < 0) | (cbp_index >= S.shape[-1])
            if bool(bad.any()):
                self._host_err = True
            cbp_acc = _host_pair_accuracy(S_pred, cbp_mask, cbp_index.masked_fill(bad, 0), self.na_canonical_base_pair_ints)
            cbp_acc = cbp_acc.masked_fill(bad, 0)
            loss, _ = train.loss_smoothed(S, log_probs, mask_for_loss, loss_masks, polymer_restype_masks, polymer_restype_nums,
                                          weight=weight, num_letters=log_probs.shape[-1], ppm_mask=ppm_mask, aligned_ppm=aligned_ppm)
            return self._accumulate_host(loss, accuracy, cbp_acc, cbp_mask, S, S_pred, train_or_valid, mask_for_loss, polymer_masks,
                                         interface_masks)
        V = log_probs.shape[-1]
        keep = []
        m = _batch(S, cbp_mask, cbp_index, V, keep, log_probs)
        m.pair_bits = _pair_bits(self.na_canonical_base_pair_ints, V)
        keys = ("protein", "dna", "rna")
        for k, key in enumerate(keys):
            m.loss_polymer[k] = _ref(loss_masks[key], keep)
            rm = polymer_restype_masks[key].contiguous().float()
            keep.append(rm)
            m.restypes[k] = rm.data_ptr()
            m.eps_scale[k] = float(np.float32(weight / polymer_restype_nums[key]))      # float32, as train.loss_smoothed
        m.weight = float(weight)
        if ppm_mask is not None:
            m.ppm_mask = _ref(ppm_mask, keep)
            ppm64 = aligned_ppm.contiguous().to(torch.float64)
            keep.append(ppm64)
            m.aligned_ppm = ppm64.data_ptr()
        self._launch(m, keep, train_or_valid, mask_for_loss, polymer_masks, interface_masks, log_probs.device)

    def _accumulate_host(self, loss, accuracy, cbp_acc, cbp_mask, S_true, S_pred, train_or_valid, mask_for_loss, polymer_masks,
                         interface_masks):
        table = self.metrics
        col = self.metric_to_col
        for polymer in [""] + list(polymer_masks):
            for interface in [""] + list(interface_masks):
                name, mask = train_or_valid, mask_for_loss
                if polymer:
                    name, mask = name + "_" + polymer, mask * polymer_masks[polymer]
                if interface:
                    name, mask = name + "_" + interface, mask * interface_masks[interface]
                r = self.mask_to_row[name]
                sums = {"weights": mask, "canonicalBasePairWeights": mask * cbp_mask, "loss": loss * mask, "accuracy": accuracy * mask,
                        "canonicalBasePairAccuracy": cbp_acc * mask * cbp_mask}
                for q, c in zip(_QUANTITIES, self._col_of):
                    if c >= 0:
                        table[r, c] += torch.sum(sums[q]).item()
                for res_name, res in zip(self.count_metrics, self._res):
                    table[r, col["true" + res_name]] += torch.sum((S_true == res).long() * mask).item()
                    table[r, col["pred" + res_name]] += torch.sum((S_pred == res).long() * mask).item()

    def all_reduce(self, group=None):
        """Sum the table over the ranks of ``group`` with one all-reduce (data-parallel training: every rank accumulated its own
        batches).  Call it on every rank before ``compute_metrics``."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        t = self._dev if self._dev is not None else torch.from_numpy(self._host)     # the numpy table is reduced in place
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def compute_metrics(self):
        """Normalise the sums by their weight columns (NaN where a weight is 0) and fill the perplexity = exp(mean loss).  Raises
        ValueError if a batch carried a canonical_base_pair_index outside [0, L)."""
        if self._host_err or (self._err is not None and bool(self._err.any())):
            raise ValueError("canonical_base_pair_index outside [0, L) in an accumulated batch (those tokens counted as no pair)")
        table = self.metrics
        col = self.metric_to_col
        normalised = [(m, w) for m, w in self.sum_metrics.items()]
        for m, w in self.count_metrics.items():
            normalised += [("true" + m, w), ("pred" + m, w)]
        for m, w in normalised:
            weights = table[:, col[w]]
            zero = weights == 0
            table[zero, col[m]] = np.nan
            table[~zero, col[m]] = table[~zero, col[m]] / weights[~zero]
        if "perplexity" in self.extra_metrics:
            table[:, col["perplexity"]] = np.exp(table[:, col["loss"]])

    def create_print_string(self, e, step, train_time, valid_time):
        table = self.metrics
        parts = [f"epoch: {e+1}, step: {step}, train_time: {train_time}, valid_time: {valid_time}"]
        for r in range(len(self.row_to_mask)):
            for metric in self.metric_names:
                value = np.format_float_positional(np.float32(table[r, self.metric_to_col[metric]]), unique=False, precision=3)
                parts.append(f"{self.row_to_mask[r]}_{metric}: {value}")
        return ", ".join(parts)

    def masks_for(self, feature_dict):
        """(polymer_masks, interface_masks) of this manager's rows from a feature_dict, as na_run.py:209-214 builds them:
        ``<name>_mask`` per polymer, ``interface`` = interface_mask and ``nonInterface`` = 1 - interface_mask."""
        polymer = {k: feature_dict[k + "_mask"] for k in self.polymer_mask_names}
        interface = {}
        for k in self.interface_mask_names:
            interface[k] = feature_dict["interface_mask"] if k == "interface" else 1 - feature_dict["interface_mask"]
        return polymer, interface


_COUNTS = ["DA", "DC", "DG", "DT", "A", "C", "G", "U"]
_MODES = {
    "basic": dict(dataset_names=["train", "valid"], polymer_mask_names=["protein", "dna", "rna"], interface_mask_names=[],
                  sum_metrics={"loss": "weights", "accuracy": "weights", "canonicalBasePairAccuracy": "canonicalBasePairWeights"},
                  count_metrics={}),
    "all": dict(dataset_names=["train", "valid"], polymer_mask_names=["protein", "dna", "rna"], interface_mask_names=["interface", "nonInterface"],
                sum_metrics={"loss": "weights", "accuracy": "weights", "canonialBasePairAccuracy": "canonicalBasePairWeights"},   # sic
                count_metrics={r: "weights" for r in _COUNTS}),
    "na_only_inference": dict(dataset_names=["valid"], polymer_mask_names=["dna", "rna"], interface_mask_names=[],
                              sum_metrics={"loss": "weights", "accuracy": "weights", "canonicalBasePairAccuracy": "canonicalBasePairWeights"},
                              count_metrics={r: "weights" for r in _COUNTS}),
}


def generate_metric_manager(restype_to_int, metrics_to_compute="basic"):
    """na_metric_manager.generate_metric_manager: "basic" (both shipped training configs), "all" (+ interface rows and residue counts;
    its canonical-pair accuracy column keeps the reference's misspelt, never-filled name) or "na_only_inference"."""
    cfg = _MODES[metrics_to_compute]
    return MetricManager(restype_to_int, ["weights", "canonicalBasePairWeights"], dict(cfg["sum_metrics"]), dict(cfg["count_metrics"]),
                         ["perplexity"], list(cfg["dataset_names"]), list(cfg["polymer_mask_names"]), list(cfg["interface_mask_names"]))
