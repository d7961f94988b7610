"""Static execution plan of a net over pre-allocated HBM buffers.

``Engine`` turns a linked ``Net`` (lib/net_types.py) into lists of launches of
the HIP kernels behind the C ABI (include/mpnn_hip.h).  Everything a training
step needs lives in a handful of flat device buffers:

* ``P`` / ``A`` / ``G``: parameters, momentum accumulators, gradients (fp32, one
  flat buffer each, same layout; ``G`` carries the per-node TALR statistics at
  its tail so ONE all-reduce serves data-parallel training);
* ``S``: BatchNorm moving averages (non-trainable state);
* per block and scale: the pre-BatchNorm conv sums ``s`` (the only activation
  that is materialised -- BatchNorm+ReLU are applied by consumers on load) and
  one gradient buffer that holds dz, then g, in place;
* fp64 arenas for BatchNorm statistics (forward sums, backward reductions).

There is no CPU fallback: constructing an Engine loads libmpnn_hip.so and needs
a GPU.  PyTorch provides device memory, streams and (optionally) graph capture.

Reference semantics restated here (graph structure only; arithmetic is in the
kernels): tree walk of Net.link (net_types.py:56-63), MultiscaleConvMax's
negative indexing of the input pyramid (layer_types.py:163,181-185), the
parameter -> tree-node map of minimize_expectation (net_types.py:28-34).

The engine is assembled from pieces (one module each): Structure (lib/_eng_structure.py: tree classification, kernel
families and buffer layout -- host arithmetic only, constructible on its own without a GPU), Allocation (lib/_eng_alloc.py:
the flat buffers and the layout's tables on the device),
Planner (lib/_eng_planner.py: the training program), EvalPrograms (lib/_eng_eval.py: dense and routed evaluation), Runner
(lib/_eng_run.py: staging, eager launches, hipGraph capture / replay, the interface other modules use),
StreamedPredict (lib/_eng_stream.py: 8-bit inputs, predict_all), DataParallelSections (lib/_eng_dp.py), KStepGraphs (lib/_eng_ksteps.py: K steps per graph) and Inspection
(lib/_eng_inspect.py: timings, result views, statistics).  Every asynchronous upload from pinned host memory goes through
lib/_upload.py.  The state these pieces share is declared in Engine.__init__ (or the _init_* helper of the piece that owns it).
"""
import os

import torch

from lib import _hip
from lib._eng_common import (BLOCK_COMPS, CAPTURE_MODE, HEAD_COMPS, OPT_CHUNK, ROUTER_COMPS, BoundInput, _attr, _Block, _kind, _nf,   # noqa: F401
                             _Node)
from lib._eng_structure import Structure
from lib._eng_alloc import Allocation
from lib._eng_planner import Planner
from lib._eng_eval import EvalPrograms
from lib._eng_run import Runner
from lib._eng_dp import DataParallelSections
from lib._eng_ksteps import KStepGraphs
from lib._eng_inspect import Inspection
from lib._eng_stream import StreamedPredict


class Engine(Structure, Allocation, Planner, EvalPrograms, Runner, StreamedPredict, DataParallelSections, KStepGraphs, Inspection):
    def __init__(self, net, device=None, n_max=128):
        self.net = net
        self.lib = _hip.load()
        if not torch.cuda.is_available():
            raise _hip.HipError('no GPU visible: the multipath-nn hot path runs on MI355X only')
        if device is None:
            device = 'cuda:%d' % int(os.environ.get('LOCAL_RANK', '0'))
        self.dev = torch.device(device)
        torch.cuda.set_device(self.dev)
        self.n_max = self.n_max_bwd = 0
        self.use_graph = bool(int(os.environ.get('MPNN_GRAPH', '1')))     # hipGraph replay of the step (0: eager launches)
        self.multi_stream = bool(int(os.environ.get('MPNN_STREAMS', '0')))
        self.group_fwd = bool(int(os.environ.get('MPNN_FWD_GROUP', '1')))   # wavefront-grouped forward launches
        self.bwd_levels = bool(int(os.environ.get('MPNN_BWD_LEVELS', '1')))  # one backward launch per dependency level
        self.routed_min_batch = 512      # routed='auto': routed evaluation from this batch on (see Planner._program)
        self.routed_min_batch_gen = 512  # the same for a net on the general conv kernels (profiles/gen_routed_eval_sweep.txt)
        self.fold_clear = bool(int(os.environ.get('MPNN_FOLD_CLEAR', '1')))  # no clearing launch in a training step
        self._acc_clean = False          # the step's accumulators (slot sums, TALR statistics, loss) are cleared
        self._streams = []
        self._event_keep = []
        self.n_streams = 1
        self.world = 1
        self.allreduce = None            # callable(G) installed by lib/_dp.py
        self.allreduce_capturable = False  # the collective may be captured into a hipGraph (RCCL on device tensors)
        self.dp_agree = None             # callable(bool) -> bool: logical AND over the ranks (lib/_dp.py)
        self.dp_quiesce = None           # callable(): no collective of the process group is pending or being polled
        self.dp_one_graph = bool(int(os.environ.get('MPNN_DP_ONE_GRAPH', '1')))
        # data parallel with SEVERAL gradient buckets (MPNN_DP_BUCKETS > 1; the default is one, see Structure._layout):
        # compute units the backward launches that run beside a bucket's all-reduce leave to the collective's
        # workgroups (mpnn_set_reserved_cus), and whether each bucket is applied (TALR + momentum) on a side stream as
        # soon as its all-reduce has finished.  Both measured on one GPU with a stand-in for the collective
        # (tools/dp_corunner_probe.py, profiles/r04_dp_corunner.txt) and OFF by default: a co-running kernel does not
        # slow the launches it runs beside (the launches behind the bucket points are the deep small-map ones, which
        # do not fill the chip), the reservation costs 12 us per step, and every additional parallel branch of the step
        # graph stalls the main branch by ~30 us.
        self.dp_reserve_cus = int(os.environ.get('MPNN_DP_RESERVE_CUS', '0'))
        self.dp_bucket_opt = bool(int(os.environ.get('MPNN_DP_BUCKET_OPT', '0')))
        self._opt_stream = None
        self.prologue = None             # callable(stream): first launch of every training step (the input pipeline)
        self.prologue_slot = None        # callable(stream, j): the same for step j of a K-step graph (run_steps)
        # single process: the launch that ends the backward pass also applies the update (mpnn_backward_finish_opt)
        self.fuse_opt = bool(int(os.environ.get('MPNN_FUSE_OPT', '1')))
        # co-training (lib/_co.py): this net shares every launch of its training step with co_share - 1 other nets of the
        # same architecture -- the planner budgets workgroups against resident slots / co_share and every backward
        # launch takes the table-driven (level) form, whose records the co-trainer concatenates over the nets
        self.co_share = 1
        self._keep = []
        # Dropout in front of exit classifiers (csrc/dropout.hip): the training-step counter the masks are drawn with (every
        # training step advances it, evaluation never does; Runner.dropout_step) and the data-parallel rank, which offsets
        # the layers' seeds (lib/_dp.py sets it)
        self._dropout_step = 0
        self.dropout_rank = 0
        self._init_stream_state()
        self._init_kstep_state()
        self._progs = {}
        self._graphs = {}
        self._gen = 0                    # buffer generation: counts the reallocations (Runner.generation)
        self._hyp_epoch = 0              # counts the uploads / rewrites of the device `hyp` row (Runner.hyp_epoch)
        self._reserved = 0               # compute units the library's grids leave free right now (Runner._set_reserve)
        self._last_fold = False          # the last training step left its slot sums in dsum_last (Runner.batch_stat_sums)
        self._stat_part = self._stat_ticket = None       # mpnn_route's per-workgroup partial sums (Planner)
        self._views_key = None           # (n, generation) the result views were bound for (Inspection._bind_views)
        self._sums_cache = None          # index tensors of Inspection.state_sums
        self._draw_bufs = {}             # id(dataset) -> the record buffers and upload rings lib/data.py stages this engine's draws in
        self._classify()
        self._layout()
        self._alloc_params()
        self.init_params(net.hypers.__dict__.get('seed'))
        self._ensure_capacity(n_max)
        self.last_n = 0
        self.last_mode = 'ev'
