"""The one import name of the host-side modules: everything is defined in a sibling module and re-exported here unchanged -- _ffi (what
goes to the C ABI), dycore, exchange (halo and all-reduce transports), mlp (the surrogate network), microphysics, surrogate_eval (banks,
evaluators, committees), rollout (members beside Kessler, teacher, harvester, scorer), column (sponge layer, nudger), ncio (NetCDF files),
city (simple_city's modules), sampling (statistics and training samples) and experiments (set-up sequences and step functions)."""
from . import capi  # noqa: F401
from ._ffi import _field_ptr_array, _ptr, _stream_ptr  # noqa: F401
from .capi import MWError, check  # noqa: F401
from .city import Horizontal_Sponge, Time_Averager  # noqa: F401
from .column import ColumnNudger, set_column_strict, sponge_layer  # noqa: F401
from .coupler import Coupler, endrun  # noqa: F401
from .dycore import DEFAULT_OPTIONS, PATH_LOG, Dynamics_Euler_Stratified_WenoFV, perturb_temperature  # noqa: F401
from .exchange import (install_exchange, use_rccl_allreduce, use_rccl_exchange, use_rccl_self_exchange,  # noqa: F401
                       use_torch_distributed_exchange)
from .experiments import make_simple_city, make_supercell, simple_city_step, supercell_step  # noqa: F401
from .microphysics import Microphysics_Kessler, Microphysics_Kessler_Surrogate  # noqa: F401
from .mlp import (FORM_MARKER, FORMS, SurrogateModel, _PonniLayer, load_h5_weights, load_surrogate_bank, load_surrogate_model,  # noqa: F401
                  load_surrogate_weights, mlp_forward, mlp_stencil_forward, ponni_forward, stencil_features)
from .ncio import NcFile as _NcFile  # noqa: F401
from .ncio import dycore_output  # noqa: F401
from .rollout import (RAIN_COUNTS, RAIN_FIELDS, ROLLOUT_FIELDS, ROLLOUT_IN5, ROLLOUT_STATS, ROLLOUT_WATER, Microphysics_Rollout, RainScorer,  # noqa: F401
                      RolloutHarvester, RolloutScorer, fields_divergence, kessler_members_teacher, member_column_water, member_divergence,
                      member_rain_table, member_surface_rain, rain_report, rain_scores, rain_thresholds, rollout_member_names, rollout_report)
from .rollout import box_json, domain_report  # noqa: F401
from .rollout import member_water_fix, water_fix_report  # noqa: F401
from .microphysics import water_fix_finish  # noqa: F401
from .rollout import heat_closure_report, member_heat_closure  # noqa: F401
from .microphysics import heat_closure_finish  # noqa: F401
from .rollout import SAMPLE_CLASSES, harvest_outside_report, harvest_thresholds, member_sample_mask_domain  # noqa: F401
from .mlp import load_training_domain, load_training_domains  # noqa: F401
from .sampling import DataGenerator, StatisticsGatherer  # noqa: F401
from .surrogate_eval import (EVAL_CLASSES, EVAL_FIELDS, CommitteeEvaluator, CommitteeGuard, SurrogateBank, SurrogateEvaluator, _sums_to_float,  # noqa: F401
                             committee_score, guard_config, json_safe, range_error_correlation, surrogate_scores)
from .surrogate_eval import DOMAIN_CLASSES, domain_box, domain_config, member_domain  # noqa: F401
from .surrogate_eval import EVAL_SIDES, DomainSplitEvaluator, domain_scores, domain_split_report, eval_domain_config  # noqa: F401
