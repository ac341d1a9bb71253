"""The slice of the reference's yacs config the VETO predictor reads
(pysgg/config/defaults.py:296-345,847-864; configs/VETO_final.yaml:57-81,135-154).

`CfgNode` is an attribute-access dict so that either this object or the reference's own frozen
yacs `cfg` can be handed to the predictor constructors."""
import copy


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)


def default_config():
    c = CfgNode()
    c.MODEL = CfgNode()
    c.MODEL.DEVICE = "cuda"
    rh = c.MODEL.ROI_RELATION_HEAD = CfgNode()
    rh.PREDICTOR = "VETOPredictor"
    rh.USE_GT_BOX = True
    rh.USE_GT_OBJECT_LABEL = True
    rh.POOLER_RESOLUTION = 8                      # VETO_final.yaml:57; 4 * PATCH_SIZE (predictor.SUPPORTED_PATCH_GRIDS)
    rh.MAX_PROPOSAL_PAIR = 2048
    rh.BATCH_SIZE_PER_IMAGE = 1024                # VETO_final.yaml:64
    rh.POSITIVE_FRACTION = 0.25                   # VETO_final.yaml:65
    rh.NUM_SAMPLE_PER_GT_REL = 4                  # defaults.py:352
    rh.REQUIRE_BOX_OVERLAP = False                # VETO_final.yaml:60
    rh.FEATURE_EXTRACTOR_MINI = "VETOFeatureExtractor"   # VETO_final.yaml:71
    rh.CONTEXT_HIDDEN_DIM = 512
    rh.CONTEXT_POOLING_DIM = 4096
    vt = rh.VETOTRANSFORMER = CfgNode()
    vt.PATCH_SIZE = 2
    vt.T_INPUT_DIM = 576
    vt.ENC_LAYERS = 6
    vt.NHEADS = 6
    vt.EMB_DROPOUT = 0.35
    vt.T_DROPOUT = 0.35
    rpn = c.MODEL.RPN = CfgNode()                 # what veto_amd.rpn.make_anchor_generator reads, as VETO_final.yaml:17-21 sets it
    rpn.USE_FPN = True
    rpn.ANCHOR_SIZES = (32, 64, 128, 256, 512)
    rpn.ANCHOR_STRIDE = (4, 8, 16, 32, 64)
    rpn.ASPECT_RATIOS = (0.23232838, 0.63365731, 1.28478321, 3.15089189)
    rpn.STRADDLE_THRESH = 0                       # defaults.py:161 (the yaml leaves it)
    c.MODEL.ROI_HEADS = CfgNode()
    c.MODEL.ROI_HEADS.FG_IOU_THRESHOLD = 0.5      # defaults.py:202
    c.MODEL.ROI_HEADS.BG_IOU_THRESHOLD = 0.3      # defaults.py:205
    c.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS = (10., 10., 5., 5.)   # defaults.py:209
    c.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 256  # defaults.py:214 (the box head's budget, not the relation head's)
    c.MODEL.ROI_HEADS.POSITIVE_FRACTION = 0.25    # defaults.py:216
    bh = c.MODEL.ROI_BOX_HEAD = CfgNode()
    bh.FEATURE_EXTRACTOR = "FPN2MLPFeatureExtractor"       # VETO_final.yaml:41 (the detector's own box head)
    bh.POOLER_SCALES = (0.25, 0.125, 0.0625, 0.03125)      # VETO_final.yaml:39
    bh.POOLER_SAMPLING_RATIO = 2                           # VETO_final.yaml:40
    c.DATASETS = CfgNode()
    c.DATASETS.USE_DEPTH = True
    c.GLOBAL_SETTING = CfgNode()
    c.GLOBAL_SETTING.DATASET_CHOICE = "VG"
    c.GLOBAL_SETTING.USE_BIAS = True
    c.GLOBAL_SETTING.BETA_LOSS = False
    c.GCL_SETTING = CfgNode()
    c.GCL_SETTING.GROUP_SPLIT_MODE = "divide4"
    c.GCL_SETTING.ZERO_LABEL_PADDING_MODE = "rand_insert"      # or "rand_choose" / "all_include" (VETO_final.yaml): all three are built
    c.ENSEMBLE_LEARNING = CfgNode()
    c.ENSEMBLE_LEARNING.ENABLED = False
    c.ENSEMBLE_LEARNING.TYPE = ["group"]
    c.ENSEMBLE_LEARNING.EXPERT_GROUP = False      # VETO_final.yaml:154
    c.ENSEMBLE_LEARNING.VOTING = "C"              # defaults.py:863
    c.TEST = CfgNode()
    c.TEST.RELATION = CfgNode()
    c.TEST.RELATION.LATER_NMS_PREDICTION_THRES = 0.3
    c.TEST.RELATION.REQUIRE_OVERLAP = False       # VETO_final.yaml:133
    c.GLOVE_DIR = ""
    so = c.SOLVER = CfgNode()                      # what veto_amd.solver reads, as VETO_final.yaml:95-96, 101, 125-126 sets it
    so.BASE_LR = 0.0001
    so.BIAS_LR_FACTOR = 1
    so.WEIGHT_DECAY = 1.0e-05
    so.WEIGHT_DECAY_BIAS = 0.0
    so.GRAD_NORM_CLIP = 5.0
    # veto_amd extensions (absent from the reference config; read with getattr defaults)
    c.VETO_AMD = CfgNode()
    # what the token-row Linears compute in: "mixed" (fp16 main product + e4m3 correction terms, default: 2/3 of the matrix-pipe
    # time of "precise" at 5-9e-5 logit error) | "precise" (3-term split bf16, 2-3e-5) | "fast" ("mixed" with the correction stages of the fused launches skipped, ~1.5e-3: reported only)
    c.VETO_AMD.PRECISION = "mixed"
    c.VETO_AMD.MAX_CHUNK_PAIRS = 0
    # True: eval forwards count, per layer and operand, the mixed-row elements that hit the e4m3 (448) / fp16 (65504) clamps of
    # the "mixed" mode and leave them in predictor.last_saturation (diagnostic: slower, synchronises the stream)
    c.VETO_AMD.COUNT_SATURATION = False
    c.VETO_AMD.TRAIN_FORWARD_ONLY = False         # True: .train() runs the forward + losses (no backward exists yet)
    # True: training on detected boxes (USE_GT_BOX False) samples its relation pairs with veto_detect_relsample, which has the
    # distribution of the reference's detect_relsample but not its draws for a given seed; False: sgdet training raises
    c.VETO_AMD.DEVICE_DETECT_RELSAMPLE = False
    # True: training on GT boxes (USE_GT_BOX True: predcls, sgcls) samples its relation pairs with veto_gtbox_relsample, which
    # has the distribution of the reference's gtbox_relsample but not its draws for a given seed, and needs no samp_processor;
    # False: the head uses the host code base's sampler (or an explicit one) as before
    c.VETO_AMD.DEVICE_GTBOX_RELSAMPLE = False
    # True: the training step runs in the "ordered" mode (include/veto_amd.h, veto_train_opts_t.deterministic): every gradient sum
    # has a fixed order, so two steps from one state and one seed give the same bits.  Also on under
    # torch.use_deterministic_algorithms(True) and with VETO_DETERMINISTIC=1 in the environment.  Other bits than the default; more workspace.
    c.VETO_AMD.DETERMINISTIC = False
    # True: a training step whose frozen region (everything under the lowest layer with a trainable parameter) is in eval mode runs
    # that region through the fused inference launches (include/veto_amd.h, veto_train_plan_t.frozen_fused) and uploads only the
    # tensors that changed.  Eligibility is decided per step (predictor.last_frozen_fused); an ineligible step runs as with False.
    c.VETO_AMD.FROZEN_FUSED = False
    return c
