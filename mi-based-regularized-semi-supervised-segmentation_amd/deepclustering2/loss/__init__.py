from .kl_losses import Entropy, KL_div  # noqa: F401
from .dice_loss import GeneralizedDiceLoss, MetaDice, dice_batch, dice_coef  # noqa: F401
